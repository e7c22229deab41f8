/*
 * musica.h — C ABI of libmusica_hip.so, the MI355X-native replacement for the
 * MUSICA Laplacian-pyramid contrast-amplification path of the reference
 * (class VulkanProcessing, include/vk_processing.h:26-356 of the reference;
 * dispatch script src/vk_processing.cpp:2104-2601; shaders/X.comp).
 *
 * The reference has no extern "C" surface: its harness crosses a process
 * boundary (`maverick-standalone <raw> <bmp>`, test/standalone/main.cpp:30-87)
 * that makes four C++ calls on VulkanProcessing. Each entry point below names
 * the C++ member it replaces. `bool` becomes `int` (1 = ok, 0 = failed) so the
 * reference's truthiness convention (ASSERT_MSG(call, msg)) carries over; on
 * failure a message "MUSICA ERROR: ..." is written to stderr, mirroring
 * `fprintf(stderr, "VK STATE ERROR: %s\n")` (src/vk_processing.cpp:14-18), and
 * is retrievable with musica_last_error().
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * All images are square (the reference never handles W != H,
 * src/vk_processing.cpp:2630-2631), single channel, row-major, dense when they
 * cross the ABI (the library keeps its own pitched layout in HBM).
 */
#ifndef MUSICA_H
#define MUSICA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUSICA_ABI_VERSION 3

/* Hard-coded constants of the reference. */
#define MUSICA_MAX_LEVELS 16          /* reference: 12 + 1 clear buffers, vk_processing.h:67 */
#define MUSICA_MIN_LEVELS 4           /* cnrLevel = coarserLevelsStart = 3 must exist, vk_processing.h:28-29 */
#define MUSICA_NOISE_BINS 2048        /* vk_processing.h:37, noise_hist.comp:6 */
#define MUSICA_GRAD_BINS 1024         /* vk_processing.h:38, gradation_histogram.comp:6 */
#define MUSICA_MAX_POINTS 256         /* contrast_curve_generate.comp:5 */
#define MUSICA_CNR_LEVEL 3            /* vk_processing.h:29 */
#define MUSICA_COARSER_LEVELS_START 3 /* vk_processing.h:28 */
#define MUSICA_OUT_MARGIN 10          /* src/vk_processing.cpp:2607 */
#define MUSICA_CLAHE_TILES 4          /* clahe_histogram.comp:4 */
#define MUSICA_CLAHE_BINS 256         /* clahe_grad_curve.comp:4 */

/* T1: struct HistogramMaxPoint, vk_processing.h:123-126. */
typedef struct musica_hist_max_point {
    uint32_t maxValue;
    uint32_t maxBin;
} musica_hist_max_point;

/* T2: struct ContrastParameters, vk_processing.h:135-138. */
typedef struct musica_contrast_params {
    float lowContrastFactor;
    float highContrastFactor;
} musica_contrast_params;

typedef struct musica_point {
    float x;
    float y;
} musica_point;

/* T3: struct ContrastCurveObj, vk_processing.h:141-149 (2052 bytes). */
typedef struct musica_contrast_curve {
    musica_point points[MUSICA_MAX_POINTS];
    uint32_t pointsCount;
} musica_contrast_curve;

/* T4: struct NoiseReductionParams, vk_processing.h:112-117. */
typedef struct musica_nr_params {
    float lowCnr;
    float lowFactor;
    float highCnr;
    float highFactor;
} musica_nr_params;

/* T5: struct GradCurveObj, vk_processing.h:215-222 (2064 bytes). */
typedef struct musica_grad_curve {
    musica_point points[MUSICA_MAX_POINTS];
    uint32_t pointsCount;
    float t0;
    float ta;
    float t1;
} musica_grad_curve;

/* Per-image summary gathered across GPUs by the batch driver. */
typedef struct musica_stats {
    uint32_t image_id;        /* index inside the batch handed to execute */
    float min_sqrt;           /* final texel of the min chain (min_reduce.comp) */
    float max_sqrt;           /* final texel of the max chain (img_max_reduce.comp) */
    uint32_t noise_max_bin[4];   /* HistogramMaxPoint.maxBin of levels 0..3 */
    uint32_t noise_max_value[4]; /* HistogramMaxPoint.maxValue of levels 0..3 */
    uint32_t grad_max_bin;
    uint32_t grad_max_value;
    float mean_cnr;           /* mean(cnr image) * 256: what test/mean_cnr/script.py:13-24 prints */
    float t0, ta, t1;         /* gradation window, gradation_curve_generate.comp:54-144 */
} musica_stats;

/* Flags for musica_params.flags */
#define MUSICA_FLAG_CLAHE      0x1u /* CLAHE gradation (reference: #ifdef ENABLE_CLAHE, vk_processing.h:13) */
#define MUSICA_FLAG_NO_GRAPH   0x2u /* launch kernels eagerly instead of replaying a captured hipGraph */
#define MUSICA_FLAG_GENERIC_KERNELS 0x4u /* test hook: use the one-thread-per-texel kernels at every level */
#define MUSICA_FLAG_LINEAR     0x10u /* one in-order stream in the reference's submission order (src/vk_processing.cpp:2104-2601), replayed as a
                                        graph, whatever the workload: for contexts that run beside other contexts on one GPU (each then owns
                                        one stream = one hardware queue; musica_pipeline_* alternates steps over three of them) */
#define MUSICA_FLAG_NO_AUTOTUNE 0x8u /* skip the init-time launch-geometry autotune (rows per wavefront stay heuristic) */
#define MUSICA_FLAG_ONE_SHOT   0x40u /* the context will execute once or a few times (musica-standalone: one image per process): no autotune, no graph
                                        capture, ONE stream whatever the workload (creating a second stream costs more than one step saves).
                                        Implies NO_AUTOTUNE and NO_GRAPH; those two flags on their own do NOT change the number of streams. */
#define MUSICA_FLAG_REFERENCE_ORDER 0x20u /* the shaders' literal arithmetic order: img_smooth.comp:32-45, img_smooth_upsampled.comp:32-45
                                        (with the * 4.0 per tap) and img_sdev.comp:17-30 accumulate their 25 taps m (x) outer,
                                        n (y) inner, starting from 0. One thread per texel (as the shaders run), several times
                                        slower than the default separable order; results are bit-identical to the oracle's
                                        MUSICA_ORDER_REFERENCE. The default order is tolerance-close to this one. */

/* Construction parameters: the reference hard-wires these as literals
 * (imageSize = 3072 in test/standalone/main.cpp:31; L = ceil(log2 N) in
 * src/vk_processing.cpp:1989). */
typedef struct musica_params {
    uint32_t image_size; /* N; 16 <= N <= 16384 (a level-0 f32 plane must stay below 2 GiB: 32-bit buffer offsets) */
    uint32_t levels;     /* L; 0 => ceil(log2 N) (reference rule); else 4 <= L <= ceil(log2 N) */
    uint32_t batch;      /* images per execute call, 0 => 1 (reference: 1) */
    int32_t device;      /* HIP device ordinal */
    uint32_t flags;      /* MUSICA_FLAG_* */
} musica_params;

/* The reference's compile-time configuration of the contrast and noise-reduction parameter formulas as runtime values (ABI version 3).
 * Replaces: the private constants of include/vk_processing.h:39-49 (nrHighCnr, nrMaxHighFactor, nrLowCnr, nrMinLowFactor,
 * highContrastMaxReduction, lowContrastMaxEnhancment) and the two #defines of include/vk_processing.h:16-17
 * (LINEAR_LOW_CONTRAST_LEVELS_REDUCTION, LINEAR_HIGH_CONTRAST_LEVELS_REDUCTION) that select the linear instead of the power form of
 * src/vk_processing.cpp:262-293. musica_tunables_default() fills in the reference's values (both #defines are commented out there).
 * coarserLevelsStart = 3 and cnrLevel = 3 (vk_processing.h:28-29) stay compile-time constants here as well
 * (MUSICA_COARSER_LEVELS_START, MUSICA_CNR_LEVEL): they decide which images and launches exist, not a formula. */
typedef struct musica_tunables {
    float nr_high_cnr;                  /* nrHighCnr = 9.0f */
    float nr_max_high_factor;           /* nrMaxHighFactor = 1.2f */
    float nr_low_cnr;                   /* nrLowCnr = 3.0f */
    float nr_min_low_factor;            /* nrMinLowFactor = 0.6f */
    float high_contrast_max_reduction;  /* highContrastMaxReduction = 0.2f */
    float low_contrast_max_enhancement; /* lowContrastMaxEnhancment = 3.0f */
    uint32_t linear_low_contrast;       /* != 0: #define LINEAR_LOW_CONTRAST_LEVELS_REDUCTION  (src/vk_processing.cpp:282-287) */
    uint32_t linear_high_contrast;      /* != 0: #define LINEAR_HIGH_CONTRAST_LEVELS_REDUCTION (src/vk_processing.cpp:262-268) */
} musica_tunables;

typedef struct musica_ctx musica_ctx;

/* Image kinds addressable by musica_get_image / musica_debug_set_image.
 * `level` is the pyramid level whose grid the image lives on. */
typedef enum musica_image_kind {
    MUSICA_IMG_NORMALIZED = 0,   /* normalizedImageState, N x N (level must be 0) */
    MUSICA_IMG_DOWNSAMPLED = 1,  /* downsampledImageStates[level], side S_{level+1} */
    MUSICA_IMG_BANDPASS = 2,     /* bandpassImageStates[level], side S_level */
    MUSICA_IMG_SDEV = 3,         /* sdevImageStates[level] (levels 0..3), side S_level */
    MUSICA_IMG_CNR = 4,          /* cnrImageState, side S_3 (level must be 3) */
    MUSICA_IMG_EXPAND = 5,       /* expandImageStates[L-1-level]: reconstruction at `level`, side S_level */
    MUSICA_IMG_GRADED = 6,       /* gradedImageState, N x N (level must be 0) */
    MUSICA_IMG_RELEVANT = 7,     /* relevantImageState, N x N; recomputed on demand (not stored on the hot path) */
    MUSICA_IMG_LOWPASS = 8,      /* lowpassImageStates[level]; recomputed on demand */
    MUSICA_IMG_EXP_BANDPASS = 9, /* band after contrast curve (+ noise reduction on levels 0,1) as fed to img_addition; recomputed on demand */
    MUSICA_IMG_SQRT = 10,        /* sqrtImageState, N x N; recomputed on demand */
    MUSICA_IMG_CLAHE_GRADED = 11, /* claheGradedImageState, N x N (only with MUSICA_FLAG_CLAHE; src/vk_processing.cpp:432-438) */
    MUSICA_IMG_CONTRAST_BAND = 12, /* expandBandpassImageStates[L-1-level]: band after the contrast curve, BEFORE noise reduction (what
                                    * debugProcess dumps as exp_bandpass_i, src/vk_processing.cpp:2710-2718); recomputed on demand */
    MUSICA_IMG_KIND_COUNT = 13
} musica_image_kind;

/* Pipeline stages runnable one at a time through musica_debug_run_stage
 * (kernel-level parity tests inject an input with musica_debug_set_image and
 * run exactly one stage). Names follow the per-stage timing line of the
 * reference (src/vk_processing.cpp:2585-2595). */
typedef enum musica_stage {
    MUSICA_STAGE_NORM = 0,   /* sqrt, min/max chains, normalize        (.cpp:2182-2222) */
    MUSICA_STAGE_REDUCE = 1, /* smooth, downsample, upsample, smooth_upsampled, difference (.cpp:2233-2273) */
    MUSICA_STAGE_ANALYSIS = 2, /* sdev, noise_hist, hist_max, contrast_curve_generate, cnr (.cpp:2284-2357) */
    MUSICA_STAGE_EXPAND = 3, /* contrast apply, noise reduction, upsample, smooth_upsampled, addition (.cpp:2361-2431) */
    MUSICA_STAGE_GRADATION = 4, /* relevant, grad hist, hist max, curve generate, curve apply (.cpp:2456-2518) */
    MUSICA_STAGE_COUNT = 5
} musica_stage;

/* ---- lifecycle ------------------------------------------------------- */

/* Replaces: VulkanProcessing::VulkanProcessing(VulkanState*) + bool init(uint32_t imageSize,
 * std::vector<VkImageView>*) (vk_processing.h:281-288, src/vk_processing.cpp:1984-2020).
 * Allocates every device buffer once; returns NULL on failure. */
musica_ctx* musica_create(const musica_params* params);
/* The same with the parameter formulas' constants given by the caller (NULL: the reference's). Values the formulas cannot use
 * (nr_high_cnr == nr_low_cnr, non-finite numbers) are refused. */
musica_ctx* musica_create_ex(const musica_params* params, const musica_tunables* tunables);
void musica_tunables_default(musica_tunables* out);
/* the tunables a context was created with */
int musica_get_tunables(const musica_ctx* ctx, musica_tunables* out);

/* Replaces: bool VulkanProcessing::cleanup() (src/vk_processing.cpp:2647-2651). Frees everything. */
void musica_destroy(musica_ctx* ctx);

/* Replaces: uint32_t getImageSize() (vk_processing.h:355). */
uint32_t musica_get_image_size(const musica_ctx* ctx);
uint32_t musica_get_levels(const musica_ctx* ctx);
uint32_t musica_get_batch(const musica_ctx* ctx);
/* Side of pyramid level `level` (S_0 = N, S_{i+1} = ceil(S_i / 2); level may be L for the residual). */
/* 1 when the level-0 expand launch of this context also accumulates the gradation histogram (no separate pass over the
 * reconstructed image; bench.py prices the launch accordingly), else 0. */
int musica_fuses_gradation_histogram(const musica_ctx* ctx);
/* 1 when level 0's smooth + downsample and band-pass image come out of one launch (k_reduce_band_u16; the `reduce_l0` profile
 * family then covers both and `band_l0` stays empty), else 0. */
int musica_fuses_reduce_band(const musica_ctx* ctx);
/* 1 when the expand launches of levels 0 .. 2 compute the 5 x 5 RMS of their band image themselves and the sdev + noise-histogram
 * launches of those levels store no image (whole-step execution only: getters, dumps and the stage entry points produce the stored
 * images on demand, bit-identical); chosen per workload by musica_create, MUSICA_SDEV_IN_EXPAND=0|1 overrides. bench.py prices
 * the launches accordingly. */
int musica_fuses_sdev(const musica_ctx* ctx);
/* How many paired launches (k_rb_sdev: the sdev + noise-histogram pass of level i and the smooth + downsample and band-pass launch of
 * level i + 1 as one launch, for i = 0, 1, ..) one whole step of this context runs; 0 when its steps run no pair (two streams, the
 * generic kernels, MUSICA_FLAG_REFERENCE_ORDER, pairing off: musica_create chooses it per workload, MUSICA_PAIR_RB_SDEV=0|1
 * overrides) or when no level qualifies (levels i and i + 1 need sides that are multiples of 8, and level i + 1 must lie above the
 * one-launch tail of small levels). Returns 0 for a NULL context. */
int musica_get_paired_levels(const musica_ctx* ctx);
/* 1 when level 0's smooth + downsample and band-pass launch of a whole step also counts the level's noise histogram from the band
 * values it has in registers (k_reduce_band_hist) and what is left of the level-0 sdev pass is the seam: the two columns either side of
 * every 512-column strip boundary, counted from the stored band image. Needs musica_fuses_sdev, raw-pixel level-0 launches and a side
 * of at least 512; chosen by musica_create for one-stream contexts whose level-0 launch fills the chip with segments of 16 coarse rows
 * (the contexts of a pipeline from 8 x 2048^2 or one 4096^2 image per step), MUSICA_HIST_IN_RB=0|1 overrides. Histograms, curves and
 * images are the same bits either way. Returns 0 for a NULL context. */
int musica_fuses_noise_hist(const musica_ctx* ctx);
uint32_t musica_get_level_size(const musica_ctx* ctx, uint32_t level);
/* How this context dispatches a step (chosen by musica_create from the batch, the image side, the depth of the pyramid and the
 * flags): *streams = 1 (the reference's one in-order queue), 2 (the analysis launches on a second stream
 * beside the reduce tail: the default for everything but small steps; MUSICA_STREAMS=1|2 overrides); *graph = 1 when steps replay a
 * captured hipGraph, 0 for eager launches. Either pointer may be NULL. Returns 1, 0 for a NULL context. */
int musica_get_dispatch(const musica_ctx* ctx, int* streams, int* graph);

/* ---- the hot path ---------------------------------------------------- */

/* Replaces: bool VulkanProcessing::execute(const uint16_t* imageData) (src/vk_processing.cpp:2104-2601).
 * `pixels`: batch * N * N host uint16, row-major, borrowed for the call
 * (H2D copy inside, as vk_state.cpp:313-342 does). Synchronous: returns after
 * the device finished, like the final vkWaitForFences (.cpp:2535-2536). */
int musica_execute(musica_ctx* ctx, const uint16_t* pixels);

/* Same pipeline with the input already resident in HBM: `d_pixels` is a device
 * pointer to batch * N * N uint16 (dense). Enqueues on the ctx stream and
 * returns without waiting; pair with musica_sync(). The dispatch script is
 * captured into a hipGraph once per distinct `d_pixels` and replayed afterwards;
 * a context keeps the graphs of the 4 most recently used pointers (rotating more
 * than 4 buffers through one context recaptures — a host-side stall of about a
 * millisecond plus a stream drain — every time a pointer comes back). */
int musica_execute_device(musica_ctx* ctx, const uint16_t* d_pixels);

/* Uploads host pixels into the ctx-owned resident input buffer and returns its
 * device pointer (for musica_execute_device). */
int musica_upload(musica_ctx* ctx, const uint16_t* pixels);
const uint16_t* musica_input_device_ptr(musica_ctx* ctx);

/* Blocks until everything enqueued on the ctx stream has finished. */
int musica_sync(musica_ctx* ctx);

/* ---- results --------------------------------------------------------- */

/* D2H of gradedImageState (f32, batch * N * N, dense) — the image
 * saveOutImage reads back (src/vk_processing.cpp:2609-2621). */
int musica_get_graded(musica_ctx* ctx, float* dst);

/* Replaces: bool VulkanProcessing::saveOutImage(std::string) (src/vk_processing.cpp:2603-2645):
 * crop MUSICA_OUT_MARGIN on every side, (uint8_t)(255.0f * v), 24-bpp bottom-up
 * BMP byte-identical to stbi_write_bmp(comp = 1) (stb_image_write.h:492-500).
 * `image_index` selects the image of the batch (reference: 0). */
int musica_save_out_image(musica_ctx* ctx, uint32_t image_index, const char* path);

/* The 8-bit cropped pixels saveOutImage would write, side N - 20, top-down rows. */
int musica_get_out_pixels(musica_ctx* ctx, uint32_t image_index, uint8_t* dst);

/* One dense f32 image of one batch entry; side = musica_image_side(kind, level). */
int musica_get_image(musica_ctx* ctx, uint32_t image_index, musica_image_kind kind, uint32_t level, float* dst);
uint32_t musica_image_side(const musica_ctx* ctx, musica_image_kind kind, uint32_t level);

/* Integer / small-struct state (bit-exact parity objects). */
int musica_get_noise_hist(musica_ctx* ctx, uint32_t image_index, uint32_t level, uint32_t* dst /*2048*/);
int musica_get_grad_hist(musica_ctx* ctx, uint32_t image_index, uint32_t* dst /*1024*/);
int musica_get_noise_hist_max(musica_ctx* ctx, uint32_t image_index, uint32_t level, musica_hist_max_point* dst);
int musica_get_grad_hist_max(musica_ctx* ctx, uint32_t image_index, musica_hist_max_point* dst);
int musica_get_contrast_curve(musica_ctx* ctx, uint32_t image_index, uint32_t level, musica_contrast_curve* dst);
int musica_get_grad_curve(musica_ctx* ctx, uint32_t image_index, musica_grad_curve* dst);
int musica_get_contrast_params(musica_ctx* ctx, uint32_t level, musica_contrast_params* dst);
int musica_get_nr_params(musica_ctx* ctx, uint32_t level /*0..2*/, musica_nr_params* dst);
int musica_get_minmax(musica_ctx* ctx, uint32_t image_index, float* min_sqrt, float* max_sqrt);
int musica_get_stats(musica_ctx* ctx, uint32_t image_index, musica_stats* dst);
/* Writes the musica_stats of every image of the batch (batch * sizeof(musica_stats) bytes,
 * image_id = image_id_base + index) into caller-owned DEVICE memory, asynchronously on the ctx
 * stream: the buffer the multi-GPU batch driver hands to its RCCL all-gather. */
int musica_stats_device(musica_ctx* ctx, void* d_dst, uint32_t image_id_base);
/* The same with image_id = image_id_base + index * image_id_stride: a rank of the batch driver owns the images
 * rank, rank + world, rank + 2 * world, ..., so its rows carry their job-wide ids without a second kernel. */
int musica_stats_device_strided(musica_ctx* ctx, void* d_dst, uint32_t image_id_base, uint32_t image_id_stride);
/* CLAHE state (only with MUSICA_FLAG_CLAHE): 4*4*256 u32 histograms [tx][ty][bin], 4*4*256 curve points. */
int musica_get_clahe_hist(musica_ctx* ctx, uint32_t image_index, uint32_t* dst);
int musica_get_clahe_curves(musica_ctx* ctx, uint32_t image_index, musica_point* dst);

/* Replaces: bool VulkanProcessing::debugProcess() (src/vk_processing.cpp:2661-2809): writes
 * norm.bmp, red_bandpass_i.bmp, red_lowpass_i.bmp, sdev.bmp, cnr.bmp,
 * exp_bandpass_i.bmp, exp_lowpass_i.bmp, relevant.bmp, graded.bmp (same
 * quantisation as VulkanState::downloadAndSaveImage, src/vk_state.cpp:809-855)
 * into `dir`, the two RGBA plots noise_hist.bmp / grad_hist.bmp, and (an addition)
 * noise_hist.csv / grad_hist.csv / grad_curve.csv with the numbers behind them. */
int musica_debug_process(musica_ctx* ctx, uint32_t image_index, const char* dir);
/* The two RGBA plots the reference renders on every execute (#define RENDER_HISTS, include/vk_processing.h:22) and
 * debugProcess writes as noise_hist.bmp / grad_hist.bmp (src/vk_processing.cpp:2758-2806): noise_hist_render.comp on the
 * histogram of cnrLevel (:1260-1266) and gradation_curve_debug_render.comp on the gradation histogram + tone curve
 * (:1668-1675), each one workgroup of 512 invocations on a histRenderWidth x histRenderHeight rgba8 image
 * (include/vk_processing.h:31-32). `rgba`: MUSICA_HIST_RENDER_WIDTH * MUSICA_HIST_RENDER_HEIGHT * 4 bytes, top row first. */
#define MUSICA_HIST_RENDER_WIDTH 512
#define MUSICA_HIST_RENDER_HEIGHT 128
int musica_render_noise_hist(musica_ctx* ctx, uint32_t image_index, uint8_t* rgba);
int musica_render_grad_hist(musica_ctx* ctx, uint32_t image_index, uint8_t* rgba);

/* ---- steps in flight (new, not in the reference) ----------------------- */

/* The reference has one VulkanProcessing and one frame in flight (vkWaitForFences at the end of execute,
 * src/vk_processing.cpp:2535-2536). A pipeline is `depth` contexts of one GPU, each created from `params` with
 * MUSICA_FLAG_LINEAR, whose steps alternate: step s is enqueued (asynchronously) on context s mod depth, so the chip-filling
 * kernels of a step run in the part-idle phases of the steps beside it (three contexts: +23 % throughput at 8 x 2048^2,
 * 2.3 x for one image per step). musica_pipeline_prime() captures every context's graph and chooses WHICH hardware queues
 * stay: it creates one context per queue of the runtime (MUSICA_PIPELINE_QUEUES), times every cyclic window of `depth` of
 * them for `calibration_steps` steps (0: three per context) and destroys the contexts outside the fastest window — two of
 * the four queues of an MI355X do not run side by side. Order of calls: create, upload (or fill every context's input
 * through musica_pipeline_context), prime, then step / sync at will. A context runs its own steps in order: the results of
 * the step a context ran last are valid after musica_sync of that context (or musica_pipeline_sync) and before its next step. */
typedef struct musica_pipeline musica_pipeline;
#define MUSICA_PIPELINE_QUEUES 4
musica_pipeline* musica_pipeline_create(const musica_params* params, uint32_t depth);
musica_pipeline* musica_pipeline_create_ex(const musica_params* params, uint32_t depth, const musica_tunables* tunables);   /* NULL: the reference's constants */
void musica_pipeline_destroy(musica_pipeline* p);
uint32_t musica_pipeline_depth(const musica_pipeline* p);
/* k-th context: before prime() k < max(depth, MUSICA_PIPELINE_QUEUES) (depth 1: one), afterwards k < depth, in step order. */
musica_ctx* musica_pipeline_context(musica_pipeline* p, uint32_t k);
/* The same batch (batch x N x N uint16, host memory) into the input buffer of every context. */
int musica_pipeline_upload(musica_pipeline* p, const uint16_t* pixels);
int musica_pipeline_prime(musica_pipeline* p, uint32_t calibration_steps);
/* ms per step of the windows prime() timed (window k starts at the k-th created context); returns how many (0: none). */
uint32_t musica_pipeline_calibration(const musica_pipeline* p, float* window_ms /* [MUSICA_PIPELINE_QUEUES] or NULL */);
/* Enqueue one step on the next context: d_pixels (device memory, 16-byte aligned) or, when NULL, that context's own input. */
int musica_pipeline_step(musica_pipeline* p, const uint16_t* d_pixels);
/* The context the most recent step was enqueued on. */
musica_ctx* musica_pipeline_last(musica_pipeline* p);
int musica_pipeline_sync(musica_pipeline* p);

/* ---- similarity metrics of the metamorphic study (new, not in the reference) ---- */

/* The reference's study scores each processed altered image against the processed unaltered one with 1 - RMSE / 255, SSIM (7 x 7
 * uniform window, K1 = 0.01, K2 = 0.03, data range 255, sample covariance, borders cropped) and three 256-bin histogram distances
 * (test/metamorphic_test/script.py:143-198; harness.py mse_similarity / ssim_similarity / hist_similarity). These entry points
 * compute them on the device: side a is the 8-bit output of a batch image (exactly what musica_get_out_pixels returns, quantised
 * while it is read), side b one of MUSICA_SIM_SLOTS context-owned reference planes of side N - 20. A region is given in
 * output-pixel coordinates: (ax, ay) in a, (bx, by) in b, w x h (w, h >= 7). All three run on the context's stream after whatever
 * was enqueued there (a step, musica_execute_device, a pipeline step of this context) and add nothing to a step. */
#define MUSICA_SIM_SLOTS 8
#define MUSICA_SIM_MAX_QUERIES 64
typedef struct musica_sim_query {
    uint32_t image_index, slot, ax, ay, bx, by, w, h;
} musica_sim_query;
typedef struct musica_sim_result {
    double mse, ssim, hist_intersection, hist_distance, hist_bhattacharyya;   /* harness.similarities' five numbers */
    uint64_t sq_diff_sum, pixels;                                             /* exact: sum of (a - b)^2 over the region, w * h */
    uint32_t bins_a[256], bins_b[256];                                        /* == np.histogram(a or b, bins=256)[0] */
    uint32_t min_a, max_a, min_b, max_b;                                      /* the values np.histogram's range spans */
} musica_sim_result;
/* The current 8-bit output of image `image_index` into `slot` (device to device). */
int musica_sim_capture(musica_ctx* ctx, uint32_t slot, uint32_t image_index);
/* (N - 20)^2 host bytes, top-down rows, into `slot` (synchronous). */
int musica_sim_set_reference(musica_ctx* ctx, uint32_t slot, const uint8_t* pixels);
/* The vendor-processed image of the raw one ((N - 20)^2 host values, top-down rows, as stored in its DICOM file: u16 when
 * bits_allocated is 16, u8 when it is 8) into `slot`, converted on the device into the 8-bit image the reference's study compares
 * against (test/metamorphic_test/script.py:396-405: Pillow's point(i * 1/256).convert('L') truncates, ImageOps.invert whatever the
 * PhotometricInterpretation): 255 - (v >> 8) for u16, 255 - v for u8 (harness.vendor_to_u8). Uploads through a context-owned staging
 * plane (allocated on first use); synchronous. Refused before any device work: NULL pointers, a slot out of range, bits_allocated
 * other than 8 or 16, an image too small for the margin. */
int musica_sim_set_vendor_reference(musica_ctx* ctx, uint32_t slot, const void* pixels, uint32_t bits_allocated /* 8 or 16 */);
/* `count` (1 .. MUSICA_SIM_MAX_QUERIES) comparisons in one launch; synchronous. Refused (0, musica_last_error) before any device work:
 * NULL pointers, a count out of range, a slot out of range or never written, image_index >= batch, a region that leaves either
 * plane, w < 7 or h < 7. */
int musica_sim_compare(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_result* results);
/* Rotates reference slot `src_slot` into `dst_slot` (device to device, on the ctx stream) as ndimage.rotate(order=0, reshape=False,
 * mode="constant", cval=0) does with the 2 x 2 `matrix` (row-major) and `offset` it computes for a plane of side N - 20
 * (harness.rotated_reference). dst_slot != src_slot; src_slot must have been written. */
int musica_sim_rotate_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, const double matrix[4], const double offset[2]);
/* Reference slot `src_slot` under element `element` (0 .. 7) of the square's symmetry group into `dst_slot` (device to device, on the
 * ctx stream): np.rot90(b if element < 4 else b.T, element & 3) of the (N - 20)^2 plane, the index table of MUSICA_ALTER_SYMMETRY with
 * side N - 20 (harness.apply_symmetry). Refused before any device work: a NULL context, a slot out of range, dst_slot == src_slot, a
 * source slot never written, element > 7, an image too small for the margin. Marks dst_slot written. */
int musica_sim_transform_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, uint32_t element);
/* ---- resolution loss: the exact binomial blur (new, not in the reference) ----
 * harness.binomial_blur(image, radius) is the contract: of a 2-D uint16 or uint8 plane, with a radius r in 1 .. MUSICA_BLUR_MAX_RADIUS,
 *   weights   w_k = C(2r, k), k = 0 .. 2r; they sum to 4^r
 *   borders   indices clamped (edge replicated), no fill value
 *   out[y, x] = (sum_i sum_j w_i w_j in[clamp(y + i - r), clamp(x + j - r)] + 2^(4r - 1)) >> 4r
 * ONE rounding, after the full 2-D sum, halves rounded up; no rounding between the two passes. The result has the input's type; a
 * constant plane is preserved, so nothing saturates. Every intermediate is an exact integer, which is where the largest radius comes
 * from: the row pass of u16 data needs 16 + 2r <= 32 bits, so it fits u32 exactly up to r = 8; the full sum needs 16 + 4r <= 48 bits
 * (u64). At r = 8 the blur is a Gaussian of sigma = sqrt(r / 2) = 2 pixels. The device results are bit-identical to that statement and
 * repeat from call to call (kernels_blur.hip). */
#define MUSICA_BLUR_MAX_RADIUS 8
/* binomial_blur(reference slot `src_slot`, radius) of the (N - 20)^2 u8 plane into `dst_slot` (device to device, on the ctx stream).
 * Refused before any device work: a NULL context, a slot out of range, dst_slot == src_slot, a source slot never written, a radius outside
 * 1 .. MUSICA_BLUR_MAX_RADIUS, an image too small for the margin. Marks dst_slot written; changes no other slot. */
int musica_sim_blur_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, uint32_t radius);
/* ---- lossy compression: the exact 8 x 8 block codec (new, not in the reference) ----
 * metrics.block_codec(plane, table, origin) is the contract: of a square 2-D uint16 (bits = 16) or uint8 (bits = 8) plane, with a table
 * of 64 quantiser steps Q[v][u] in 1 .. 65535 (v the vertical frequency) and an origin (oy, ox), each 0 .. 7: the plane lies on a grid of
 * 8 x 8 blocks that start at x = -ox and y = -oy (mod 8); a block that sticks out of the plane is completed by edge replication, as
 * JPEG does, and only in-plane pixels are written. Per block, in int32 throughout, rs(t, s) = (t + 2^(s - 1)) >> s (arithmetic shift),
 * M[0][x] = 512, M[u][x] = rint(512 sqrt 2 cos((2x + 1) u pi / 16)) (the 64 literals stand in kernels_codec.hip and metrics.CODEC_M):
 *   X  = v - 2^(bits - 1)
 *   A  = rs(X M^T, 10)                          rows        |X M^T| <= 2^27
 *   F  = rs(M A, 11)                            columns     |M A| <= 2^29, |F| <= 2^18  (the orthonormal DCT, DC = 8 mean exactly)
 *   q  = sign(F) ((|F| + (Q >> 1)) div Q)       halves away from zero
 *   F' = q Q                                    |F'| <= 2^18 + 32767
 *   A' = clamp(rs(M^T F', 10), -2^18, 2^18 - 1) |M^T F'| <= 3825 (2^18 + 32767) < 2^31; the clamp is part of the contract
 *   X' = rs(A' M, 11)                           |A' M| <= 2^30
 *   out = clamp(X' + 2^(bits - 1), 0, 2^bits - 1)
 * A constant block comes back exactly whenever Q[0][0] divides 8 X. The device results are bit-identical to that statement and repeat
 * from call to call (kernels_codec.hip). */
/* block_codec(reference slot `src_slot`, table, (origin, origin)) of the (N - 20)^2 u8 plane into `dst_slot` (device to device, on the
 * ctx stream); the study passes origin = MUSICA_OUT_MARGIN % 8, so the blocks lie where the raw plane's lay. Refused before any device
 * work: a NULL context, a NULL table, a slot out of range, dst_slot == src_slot, a source slot never written, a table entry of 0,
 * origin > 7, an image too small for the margin. Marks dst_slot written; changes no other slot. */
int musica_sim_codec_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, const uint16_t table[64], uint32_t origin);
/* ---- magnification: the exact rational zoom (new, not in the reference) ----
 * harness.zoom(image, (p, q)) is the contract: a square 2-D uint16 or uint8 plane of side n magnified by p / q about its centre,
 * bilinearly, in integers, with 1 <= q < p <= MUSICA_ZOOM_MAX_P and gcd(p, q) = 1. With D = 2p, for an output index x
 *   n_x = (2x - (n - 1)) q + (n - 1) p        (>= 0; the source coordinate is n_x / D)
 *   i_x = n_x div D,   f_x = n_x mod D,   g_x = D - f_x,   i+ = min(i + 1, n - 1)
 *   out[y, x] = (g_y g_x in[i_y, i_x] + g_y f_x in[i_y, i_x+] + f_y g_x in[i_y+, i_x] + f_y f_x in[i_y+, i_x+] + D^2 / 2) div D^2
 * ONE rounding, after the full 2-D sum, halves rounded up. The result has the input's type. The weights sum to D^2 <= 4096 and the sum
 * is at most 65535 * 4096 + 2048 < 2^32, so every intermediate fits u32 and a constant plane is preserved. A zoom above 1 about the
 * centre reads only inside the plane, so there is no fill value: i_x <= n - 2 except where f_x = 0, and there the clamped neighbour's
 * weight is 0. Mirroring x -> n - 1 - x maps n_x -> 2p (n - 1) - n_x, so the map commutes exactly with the eight symmetries of the
 * square; and because 2 (x + 10) - (N - 1) = 2x - (M - 1) for M = N - 20, the zoom of the cropped output plane is the crop of the zoom
 * of the full frame. The device results are bit-identical to that statement and repeat from call to call (kernels_zoom.hip; DESIGN.md
 * section 4). */
#define MUSICA_ZOOM_MAX_P 32
/* zoom(reference slot `src_slot`, (p, q)) of the (N - 20)^2 u8 plane into `dst_slot` (device to device, on the ctx stream). Refused
 * before any device work: a NULL context, q = 0, p <= q, p > MUSICA_ZOOM_MAX_P, gcd(p, q) != 1, a slot out of range, dst_slot ==
 * src_slot, a source slot never written, an image too small for the margin. Marks dst_slot written; changes no other slot. */
int musica_sim_zoom_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, uint32_t p, uint32_t q);
/* ---- scatter: the exact wide veiling glare (new, not in the reference) ----
 * harness.scatter(image, (R, a, b)) is the contract: a square 2-D uint16 or uint8 plane mixed with a very wide blur of itself, the veil
 * of scattered radiation under automatic exposure control, at the scatter fraction a / b. 1 <= R <= MUSICA_SCATTER_MAX_RADIUS,
 * 1 <= a < b <= MUSICA_SCATTER_MAX_DEN, gcd(a, b) = 1. With box(A)[i] = sum_{k = -R .. R} A[clamp(i + k)] along one axis, clamped to the
 * plane (edge replicated; each pass clamps its own input),
 *   V   = box_y(box_y(box_x(box_x(image))))              tent x tent, total weight W = (2R + 1)^4
 *   out = ((b - a) W image + a V + (b W) div 2) div (b W)
 * ONE rounding, after the full sum, halves rounded up; nothing is rounded between the passes. The result has the input's type.
 *   - the row and column operators commute: the order of the four passes changes nothing;
 *   - after the two row passes a value is at most 255^2 * 65535 = 4 261 413 375 < 2^32: the row-pass plane is u32;
 *   - W <= 255^4 = 4 228 250 625 < 2^32;
 *   - the full numerator is at most 65535 * 64 * 255^4, about 1.77e16 < 2^64: the column passes and the mix are u64;
 *   - the weights are a convex combination: a constant plane is preserved, nothing saturates, nothing is clipped;
 *   - the operator commutes exactly with the eight symmetries of the square;
 *   - it does NOT commute with cropping (the borders are clamped): a registered comparison is inset by 2R;
 *   - the tent has sigma = sqrt(2R (R + 1) / 3) pixels, 104 at R = 127.
 * The device results are bit-identical to that statement and repeat from call to call: integers only, no atomics, prefix sums along the
 * rows and running sums down the columns (kernels_scatter.hip). The first call of either entry point allocates
 * one N x N u32 plane, freed with the context. */
#define MUSICA_SCATTER_MAX_RADIUS 127
#define MUSICA_SCATTER_MAX_DEN 64
/* scatter(reference slot `src_slot`, (radius, num, den)) of the (N - 20)^2 u8 plane into `dst_slot` (device to device, on the ctx
 * stream). Refused before any device work: a NULL context, a radius outside 1 .. MUSICA_SCATTER_MAX_RADIUS, num = 0, num >= den, den >
 * MUSICA_SCATTER_MAX_DEN, gcd(num, den) != 1, a slot out of range, dst_slot == src_slot, a source slot never written, an image too
 * small for the margin, a failed allocation of the row plane. Marks dst_slot written; changes no other slot. */
int musica_sim_scatter_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, uint32_t radius, uint32_t num, uint32_t den);
/* ---- local deformation: the exact grid warp (new, not in the reference) ----
 * Every other geometric alteration moves the whole frame rigidly or affinely; patient motion, breathing and positioning differences do
 * not. harness.warp(image, field, origin) is the contract: a square 2-D uint16 or uint8 plane of side n under a backward warp
 * out[x] = in[x + d(x)] (no holes, no folds), d given on a control grid of spacing G = MUSICA_WARP_GRID pixels. The field is M x M x 2
 * integers: field[j][i] = (dx, dy), the displacement at node (row j, column i) in units of 1 / MUSICA_WARP_UNIT pixel, every component
 * within +-MUSICA_WARP_MAX_SHIFT (16 pixels). With the origin (ox, oy), 0 <= ox, oy < G, pixel (x, y) of the plane sits at grid
 * coordinate (x + ox, y + oy); M >= ((n - 1 + max(ox, oy)) >> 6) + 2 and nodes beyond that count are ignored, so one node array serves
 * the raw plane (origin 0) and the output plane cropped by the margin (origin MUSICA_OUT_MARGIN). In integers, `>>` the arithmetic
 * shift (a floor), for output pixel (x, y):
 *   X = x + ox,  cx = X >> 6,  fx = X & 63                                       (Y, cy, fy likewise from y + oy)
 *   per component c (0: dx, 1: dy), d = field[.., .., c]:
 *     S_c = (64 - fy) ((64 - fx) d[cy, cx]     + fx d[cy, cx + 1])
 *         +       fy  ((64 - fx) d[cy + 1, cx] + fx d[cy + 1, cx + 1])           |S_c| <= 2^24
 *     s_c = (S_c + 2048) >> 12                                                   1 / 256 pixel; |s_c| <= max |d|
 *   ix = x + (s_0 >> 8),  wx = s_0 & 255                                         (iy, wy likewise from s_1)
 *   x0 = clamp(ix), x1 = clamp(ix + 1), y0 = clamp(iy), y1 = clamp(iy + 1)       clamp to 0 .. n - 1: edge replicated, no fill value
 *   out[y, x] = ((256 - wy) ((256 - wx) in[y0, x0] + wx in[y0, x1]) + wy ((256 - wx) in[y1, x0] + wx in[y1, x1]) + 32768) >> 16
 * ONE rounding of the field and ONE of the image sum, halves up; nothing is rounded between the two image passes. The sum is at most
 * 65535 * 65536 + 32768 < 2^32, so every intermediate fits i32 or u32. The result has the input's type. The sign agrees with
 * musica_sim_displace: an output that follows the input has its best shift at +d.
 *   - the zero field is the identity;
 *   - a constant field of whole pixels (256 kx, 256 ky) is in[clamp(y + ky), clamp(x + kx)] exactly, and a constant field survives the
 *     interpolation unchanged: (4096 d + 2048) >> 12 = d;
 *   - a constant plane is preserved for every field: the weights are convex, nothing saturates;
 *   - reach: r(field) = (max |d| + 255) div 256 + 1, and a pixel reads only within r of itself;
 *   - cropping commutes inside the reach: warp(P, F)[10:-10, 10:-10] and warp(P[10:-10, 10:-10], F, origin (10, 10)) agree everywhere
 *     except within r(F) of the border, where the cropped plane clamps: a registered comparison is inset by r;
 *   - no commutation with the symmetries of the square is claimed: the floors are not mirror-symmetric.
 * The device results are bit-identical to that statement and repeat from call to call (kernels_warp.hip). The
 * entry points take one origin for both axes and keep the nodes a call needs in a device buffer of the context, grown on first use. */
#define MUSICA_WARP_GRID 64
#define MUSICA_WARP_UNIT 256
#define MUSICA_WARP_MAX_SHIFT 4096
#define MUSICA_WARP_MAX_NODES 258   /* what N = 16384 needs at any origin */
/* warp(reference slot `src_slot`, field, (origin, origin)) of the (N - 20)^2 u8 plane into `dst_slot` (device to device, on the ctx
 * stream). `field`: nodes x nodes x 2 host int16, row-major, (dx, dy) per node, borrowed for the call. Refused before any device work:
 * a NULL context or field, a slot out of range, dst_slot == src_slot, a source slot never written, origin > 63, `nodes` below
 * ((N - 21 + origin) >> 6) + 2 or above MUSICA_WARP_MAX_NODES, a node component outside +-MUSICA_WARP_MAX_SHIFT (the refusal names the
 * node), an image too small for the margin. Marks dst_slot written; changes no other slot. */
int musica_sim_warp_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, const int16_t* field, uint32_t nodes, uint32_t origin);
/* (N - 20)^2 bytes of reference slot `slot` to the host (synchronous); the slot must have been written. */
int musica_sim_get_reference(musica_ctx* ctx, uint32_t slot, uint8_t* dst);

/* Tone metrics from the joint gray-level histogram of a comparison (harness.tone_similarities): J[a][b] counts the region pixels with
 * the value a in the batch image's 8-bit output and b in the reference slot, exactly (integer atomics: the same from call to call). The
 * numbers are computed on the host from J. With n = w * h, the marginals A_a and B_b, S_b = sum_a a J[a][b], Q_b = sum_a a^2 J[a][b],
 * all sums in ascending a, then ascending b, zero counts skipped, natural logarithms:
 *   h_a = -sum (A_a / n) ln(A_a / n), h_b and h_ab (over J) likewise;
 *   mi = sum (J / n) ln(J n / (A_a B_b));  nmi = 2 mi / (h_a + h_b), 1 when h_a + h_b == 0;
 *   SSW = sum over b with B_b > 0 of (B_b Q_b - S_b^2) / B_b and SST = (n sum_a a^2 A_a - (sum_a a A_a)^2) / n, each numerator an exact
 *   integer (128 bits), one f64 division per term;
 *   corr_ratio = 1 - SSW / SST, 1 when SST's numerator is 0 (Roche et al.: how much of a's variance a function of b explains);
 *   tone_mse = 1 - sqrt(SSW / n) / 255: the mse of musica_sim_compare after the least-squares gray-level remap of b onto a, E[a | b];
 *   tone_lut[b] = (2 S_b + B_b) / (2 B_b) in integer division (that remap, rounded half up) where B_b > 0, else b.
 * mi, nmi and corr_ratio do not change under an invertible remap of b's gray levels. */
typedef struct musica_sim_joint_result {
    double mi, nmi, corr_ratio, tone_mse;
    double h_a, h_b, h_ab;                  /* entropies, nats */
    uint64_t pixels;                        /* w * h */
    uint64_t sq_diff_sum;                   /* sum J (a - b)^2 == musica_sim_compare's */
    uint8_t tone_lut[256];
} musica_sim_joint_result;
/* `count` (1 .. MUSICA_SIM_MAX_QUERIES) joint histograms in one launch; synchronous. `joint` (may be NULL): count * 65536 counts, table
 * i at joint + i * 65536, row a, column b. The refusals of musica_sim_compare, so one query array serves both calls: refused (0,
 * musica_last_error) before any device work: NULL pointers, a count out of range, a slot out of range or never written, image_index >=
 * batch, a region that leaves either plane, w < 7 or h < 7. Changes no slot, no result of the step and no input image; its tables are
 * allocated on first use. */
int musica_sim_joint(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_joint_result* results, uint32_t* joint);
/* Where the output went: exact block matching of a comparison (harness.displacement_table). With S = 2 radius + 1, radius in
 * 1 .. MUSICA_SIM_MAX_RADIUS, side a the 8-bit output of batch image image_index (quantised while it is read, as musica_sim_compare
 * reads it) and side b the plane of reference slot `slot`, the table of a query is, for dy, dx in [-radius, radius],
 *   T[dy + radius][dx + radius] = sum over y < h, x < w of (a[ay + y][ax + x] - b[by + y + dy][bx + x + dx])^2.
 * Every candidate covers the same w * h pixels, so the b window grown by `radius` on every side must lie inside the plane: a query whose
 * grown window leaves it is refused, the caller insets its region. Tile (ty, tx) owns the region pixels [64 ty, min(h, 64 ty + 64)) x
 * [64 tx, min(w, 64 tx + 64)); its table is the same sum over those pixels and fits u32 (64 * 64 * 255^2 < 2^32). The query's table is
 * the sum of its tile tables in u64. The argmin of a table, the query's and a tile's: the smallest value, then the smallest
 * dx^2 + dy^2, then the smallest dy, then the smallest dx, so a flat tile reports (0, 0) and is not counted in tiles_off. All of it is
 * integer arithmetic: exact, and the same from call to call. */
#define MUSICA_SIM_MAX_RADIUS 16
#define MUSICA_SIM_TILE 64
typedef struct musica_sim_displace_result {
    uint64_t pixels;          /* w * h */
    uint64_t ssd_zero;        /* table entry (0, 0) == musica_sim_compare's sq_diff_sum of the same query */
    uint64_t ssd_min;         /* smallest table entry */
    int32_t  dx, dy;          /* its shift, by the tie rule above */
    uint32_t tiles_x, tiles_y;/* ceil(w / 64), ceil(h / 64) */
    uint32_t tiles_off;       /* tiles whose own argmin (same tie rule) is not (0, 0) */
} musica_sim_displace_result;
/* `count` (1 .. MUSICA_SIM_MAX_QUERIES) displacement tables in one launch; synchronous, on the context's stream after whatever was
 * enqueued there. `tables` (may be NULL): count * S^2 u64 values, table i at tables + i * S^2, row dy, column dx. `tile_tables` (may be
 * NULL): the queries' tile tables back to back in query order, tiles_y * tiles_x * S^2 u32 each, tile-row major. Refused (0,
 * musica_last_error) before any device work: a NULL ctx, queries or results, a count out of range, a radius outside
 * 1 .. MUSICA_SIM_MAX_RADIUS, a slot out of range or never written, image_index >= batch, w < 7 or h < 7, an a region that leaves the
 * output plane, a b window that, grown by the radius, leaves the plane. Changes no slot, no result of the step and no input image; its
 * device buffers are allocated on first use and sized for the call. */
int musica_sim_displace(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, uint32_t radius,
                        musica_sim_displace_result* results, uint64_t* tables, uint32_t* tile_tables);
/* At which spatial scale the output changed: multi-scale SSIM of a comparison (Wang, Simoncelli, Bovik 2003) with the 7 x 7 uniform
 * window of musica_sim_compare, in exact integers (harness.multiscale_similarities). Side a is the 8-bit output of batch image
 * image_index (quantised while it is read, as musica_sim_compare reads it), side b the plane of reference slot `slot`. For
 * s = 0 .. scales - 1, X_s[i][j] is the SUM of the 2^s x 2^s block of the a region whose top-left pixel is (i 2^s, j 2^s) of the region,
 * Y_s the same of b: planes of (h >> s) x (w >> s) integers <= 255 * 4^s, rows and columns that do not fill a block dropped (iterated
 * 2 x 2 mean pooling, times 4^s). Over all (h_s - 6)(w_s - 6) windows of 7 x 7 texels the sums Sx, Sy, Sxx, Syy, Sxy of X_s, Y_s,
 * X_s^2, Y_s^2, X_s Y_s are exact integers; ux = Sx / (49 * 4^s), uxx = Sxx / (49 * 16^s) (likewise uy, uyy, uxy: one f64 division by
 * an exact double each), vx = (49 / 48)(uxx - ux ux), vy, vxy likewise, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, and per window
 *   lum = (2 ux uy + C1) / (ux ux + uy uy + C1),  cs = (2 vxy + C2) / (vx + vy + C2),
 *   ssim = ((2 ux uy + C1)(2 vxy + C2)) / ((ux ux + uy uy + C1)(vx + vy + C2))     (scale 0: musica_sim_compare's per-pixel value).
 * ssim[s], cs[s], lum[s] are their means over the windows (only the order of that last f64 summation is the device's own: fixed, the
 * same from call to call); ssd[s] = sum (X_s - Y_s)^2 over plane s, exact (ssd[0] == musica_sim_compare's sq_diff_sum);
 * mse[s] = 1 - sqrt(ssd[s] / (h_s w_s)) / (255 * 4^s). With W = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) and w_s = W[s] / (W[0] + ..
 * + W[scales - 1]):  ms_ssim = prod over s < scales - 1 of max(cs[s], 0)^w_s, times max(ssim[scales - 1], 0)^w_(scales - 1), C pow, in
 * ascending s. Identical sides give exactly 1 everywhere. */
#define MUSICA_SIM_MAX_SCALES 5
typedef struct musica_sim_scales_result {
    uint32_t scales;                 /* as asked */
    uint64_t pixels;                 /* w * h */
    double   ms_ssim;
    double   ssim[5], cs[5], lum[5], mse[5];
    uint64_t ssd[5];                 /* exact */
    uint32_t plane_w[5], plane_h[5]; /* w >> s, h >> s */
} musica_sim_scales_result;
/* `count` (1 .. MUSICA_SIM_MAX_QUERIES) comparisons at `scales` (1 .. MUSICA_SIM_MAX_SCALES) scales each; synchronous, on the context's
 * stream after whatever was enqueued there. The full-resolution planes are read once, by a pooling launch that writes the planes of
 * every scale into context-owned scratch (allocated on first use, sized for the call); one windowed launch covers all queries and
 * scales, a fold launch sums its partials in a fixed order. Array entries at s >= scales are zero. The refusals of musica_sim_compare,
 * so one query array serves both calls: refused (0, musica_last_error) before any device work: NULL pointers, a count out of range, a
 * slot out of range or never written, image_index >= batch, a region that leaves either plane, w < 7 or h < 7; and scales outside
 * 1 .. MUSICA_SIM_MAX_SCALES, a region with min(w, h) >> (scales - 1) < 7. Changes no slot, no result of the step and no input image. */
int musica_sim_multiscale(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, uint32_t scales,
                          musica_sim_scales_result* results);
/* dst[i] = lut[src[i]] over the (N - 20)^2 plane of reference slot `src_slot` into `dst_slot` (device to device, on the ctx stream);
 * with a musica_sim_joint_result's tone_lut: the slot tone-matched to the image it was compared with. Refused before any device work: a
 * NULL context or table, a slot out of range, dst_slot == src_slot, a source slot never written, an image too small for the margin.
 * Marks dst_slot written. */
int musica_sim_remap_reference(musica_ctx* ctx, uint32_t dst_slot, uint32_t src_slot, const uint8_t lut[256]);

/* Ensemble noise statistics: per-pixel mean and variance of the output across many realisations of a noise alteration, split into bias
 * against a reference slot and noise (harness.ensemble_statistics). One comparison scores one draw and cannot tell a systematic change of
 * the output from amplified noise; the ensemble can. a_k(p), k = 1 .. K, is the 8-bit output of realisation k at output pixel p: exactly
 * the bytes musica_get_out_pixels returns (cropped by MUSICA_OUT_MARGIN, quantised while it is read). Per pixel of the (N - 20)^2 plane
 * the context keeps S1(p) = sum_k a_k(p) and S2(p) = sum_k a_k(p)^2; with K <= MUSICA_SIM_ENSEMBLE_MAX, S1 <= 261 120 and
 * S2 <= 66 585 600 fit u32. With b(p) the plane of a reference slot and a query region of n = w h pixels, all exact integers:
 *   D(p) = S1(p) - K b(p) (signed),  V(p) = K S2(p) - S1(p)^2 (>= 0),
 *   sq_bias_sum = sum D^2,  var_sum = sum V,  bias_sum = sum D,  abs_bias_max = max |D|,  var_max = max V,
 *   sq_err_sum = sum (S2 - 2 b S1 + K b^2) = sum_k sum_p (a_k - b)^2: musica_sim_compare's sq_diff_sum summed over the K realisations,
 * and K sq_err_sum == sq_bias_sum + var_sum holds exactly. sq_bias_sum <= 255^2 K^2 n and every other sum is smaller: a query with
 * 65025 K^2 w h >= 2^64 is refused (with K = 1024 that is a region of 2^44 / 65025 pixels or more, 16 448^2: beyond any plane the library accepts). The doubles are computed on the host from those integers, one
 * IEEE operation each in this order (every integer converted to double first):
 *   mean_shift = bias_sum / (K n);  bias_rms = sqrt(sq_bias_sum / (K K n));  noise_rms = sqrt(var_sum / (K (K - 1) n)), 0 when K == 1;
 *   mse = 1 - sqrt(sq_err_sum / (K n)) / 255;  bias_fraction = sq_bias_sum / (sq_bias_sum + var_sum), 0 when both are 0.
 * Tiles are musica_sim_displace's: tile (ty, tx) owns the region pixels [64 ty, min(h, 64 ty + 64)) x [64 tx, min(w, 64 tx + 64)); a tile
 * table holds two u64 per tile, (sum D^2, sum V), tile-row major, and the tile entries of a query sum to its totals. All of it is integer
 * arithmetic: exact, and the same from call to call. */
#define MUSICA_SIM_ENSEMBLE_MAX 1024
typedef struct musica_sim_ensemble_stats {
    double mean_shift, bias_rms, noise_rms, mse, bias_fraction;
    uint64_t sq_bias_sum, var_sum, sq_err_sum;
    int64_t bias_sum;
    uint64_t abs_bias_max, var_max;
    uint64_t pixels;                          /* w * h */
    uint32_t realisations;                    /* K */
    uint32_t tiles_x, tiles_y;                /* ceil(w / 64), ceil(h / 64) */
} musica_sim_ensemble_stats;
/* Zeroes the accumulators and K, on the context's stream, and drops any tracked regions (musica_sim_ensemble_track). The accumulators
 * ((N - 20)^2 words of 8 bytes) are allocated by the first call. */
int musica_sim_ensemble_reset(musica_ctx* ctx);
/* Adds the current outputs of batch images first .. first + count - 1 and sets K += count. Enqueued on the context's stream behind whatever
 * is there (a step, musica_execute_device); returns without waiting. Refused before anything is enqueued: a NULL context, count == 0 or
 * first + count > batch, N <= 20, no step has run on the context, the ensemble was never reset, K + count > MUSICA_SIM_ENSEMBLE_MAX.
 * Changes no result of the step, no input image and no slot. */
int musica_sim_ensemble_add(musica_ctx* ctx, uint32_t first, uint32_t count);
/* `count` (1 .. MUSICA_SIM_MAX_QUERIES) queries in one launch; synchronous. Side a is the ensemble: image_index is checked like the other
 * calls and not used, so one query array serves all the musica_sim_* calls. `tile_tables` (may be NULL): the queries' tile tables back to
 * back in query order, tiles_y * tiles_x * 2 u64 each. The refusals of musica_sim_compare, and: K == 0 (never reset, or nothing added since),
 * the range condition above. Changes no accumulator, no slot, no result of the step and no input image. */
int musica_sim_ensemble_result(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_ensemble_stats* results,
                               uint64_t* tile_tables);
/* The (N - 20)^2 accumulators S1 and S2 to the host, top-down rows, and K; synchronous. Any of the three pointers may be NULL. Refused when
 * the ensemble was never reset. */
int musica_sim_ensemble_get(musica_ctx* ctx, uint32_t* s1, uint32_t* s2, uint32_t* realisations);

/* The texture of the output noise: its spatial auto-covariance over integer lags, taken over the realisations of an ensemble
 * (harness.ensemble_covariance). The per-pixel statistics above say how strong the noise is; neighbour correlations, the correlation area
 * and the noise power spectrum (Wiener-Khinchin: harness.noise_power_spectrum) follow from this table. a_k(p), k = 1 .. K, is the 8-bit
 * output of realisation k at pixel p of the (N - 20)^2 plane, exactly the bytes musica_sim_ensemble_add adds. R is the radius,
 * 1 .. MUSICA_SIM_MAX_RADIUS, S = 2 R + 1. A tracked region is the a-side rectangle (ax, ay, w, h) of a musica_sim_query, n = w h. The lags
 * are d = (dx, dy) with dy = 0 .. R and dx = -R .. R: a table has (R + 1) x S entries, row dy, column dx + R. The entries with dy = 0 and
 * dx < 0 are computed by the same formula as the others; they differ from their mirror only by edge terms. All sums over p in the region;
 * p + d may leave the region but not the plane:
 *   P(d) = sum_k sum_p a_k(p) a_k(p + d)     accumulated while realisations are added
 *   U(d) = sum_p S1(p) S1(p + d)             from the ensemble's accumulators, at result time
 *   C(d) = K P(d) - U(d)                     signed 64-bit
 *        = K^2 n x (the population covariance at lag d, about the per-pixel ensemble mean).
 * Every lag covers the same n pixels, so the region grown by R to the left and to the right and by R downwards must lie inside the plane:
 * a region whose grown window leaves it is refused, the caller insets. C(0, 0) == var_sum of musica_sim_ensemble_result for the same region,
 * exactly. Tiles are musica_sim_displace's: 64 x 64, anchored at the region's origin, ragged last tiles; a tile's table is the same sum
 * over its own pixels and the tile tables of a region sum to its table. Ranges: a tile's P of one realisation is <= 64 * 64 * 255^2 =
 * 266 342 400 < 2^28, so 16 realisations fit a u32 and 17 do not (the device keeps u64 per tile); a tile's U is <= 4096 * 261 120^2 < 2^48;
 * |C(d)| <= 65025 K^2 w h, and a region with 65025 K^2 w h >= 2^63 is refused, with K = MUSICA_SIM_ENSEMBLE_MAX, the count an ensemble
 * may reach (a region of 2^43 / 65025 pixels or more, 11 630^2), so that no later add can leave the range. The doubles are computed on the
 * host from those integers, one IEEE operation each in this order (every integer converted to double first):
 *   noise_var = C(0,0) / (K (K - 1) n), 0 when K == 1;
 *   rho_x = C(1,0) / C(0,0) and rho_y = C(0,1) / C(0,0), both 0 when C(0,0) == 0;
 *   corr_area = (C(0,0) + 2 sum C(d)) / C(0,0), 1 when C(0,0) == 0: the sum over the half plane dy > 0, or dy == 0 and dx > 0, in ascending
 *   dy, then ascending dx, in f64. This is the zero-frequency noise power over the variance: 1 for white noise.
 * All the integers are exact, and the same from call to call. */
#define MUSICA_SIM_COV_MAX_REGIONS 4
typedef struct musica_sim_cov_result {
    double noise_var, rho_x, rho_y, corr_area;
    int64_t c00;                              /* C(0, 0) == musica_sim_ensemble_result's var_sum of the region */
    uint64_t pixels;                          /* w * h */
    uint32_t realisations;                    /* K */
    uint32_t radius;                          /* R */
    uint32_t tiles_x, tiles_y;                /* ceil(w / 64), ceil(h / 64) */
} musica_sim_cov_result;
/* Declares `count` (1 .. MUSICA_SIM_COV_MAX_REGIONS) tracked regions for the ensemble now starting: allowed only after
 * musica_sim_ensemble_reset and before the first add (K == 0). Uses ax, ay, w and h of each query; the other fields are checked as
 * musica_sim_ensemble_result checks them, so the study's query arrays serve. While regions are tracked, every musica_sim_ensemble_add also
 * enqueues the product launch for the same images, on the same stream behind the accumulation. musica_sim_ensemble_reset drops the
 * tracking. The u64 tile tables are allocated on first use, sized for the call, and zeroed. Refused (0, musica_last_error) before any
 * device work: NULL pointers, a radius outside 1 .. MUSICA_SIM_MAX_RADIUS, a count out of range, an ensemble never reset or with K > 0,
 * the refusals of musica_sim_compare (w < 7 or h < 7, a region that leaves the plane, ...), a grown window that leaves the plane, the
 * range condition above. */
int musica_sim_ensemble_track(musica_ctx* ctx, uint32_t radius, uint32_t count, const musica_sim_query* regions);
/* One result per tracked region, in order; synchronous. `tables` (may be NULL): count * (R + 1) * S values C(d), table i at
 * tables + i * (R + 1) * S, row dy, column dx + R. `tile_tables` (may be NULL): the regions' tile tables C(d) back to back in region
 * order, tiles_y * tiles_x * (R + 1) * S values each, tile-row major. Refused when ctx or results is NULL, nothing is tracked or K == 0.
 * Changes no accumulator, no slot, no result of a step and no input image; may be called again after more adds. */
int musica_sim_ensemble_covariance(musica_ctx* ctx, musica_sim_cov_result* results, int64_t* tables, int64_t* tile_tables);

/* ---- alterations of the metamorphic study (new, not in the reference) ---- */

/* The study's alteration generators (harness.py apply_collimator, clamp_translation, clamp_rotate, add_gaussian_noise,
 * apply_quantum_noise; test/metamorphic_test/script.py:49-141) on the device: they read a context-owned N x N u16 source plane and
 * write one image of the resident input buffer (musica_input_device_ptr), so a study needs one upload per raw image.
 *   NONE        the source, bit-exact.
 *   TRANSLATE   clamp_translation(src, dx, dy), bit-exact, the 99th-percentile fill of its 2-pixel strip included.
 *   ROTATE      clamp_rotate: the (N - 2 margin)^2 crop rotated with `matrix` / `offset` exactly as ndimage.rotate(order=0,
 *               reshape=False, mode="constant") maps it, filled with int(np.percentile(crop, 95)); bit-exact.
 *   COLLIMATOR  apply_collimator(src, shutter_h, shutter_v): the source inside the inclusive rectangle [shutter_v, N - shutter_v] x
 *               [shutter_h, N - shutter_h], outside it min(k, 65535) with k ~ Poisson(v / 100).
 *   GAUSSIAN    add_gaussian_noise(src, mean, sigma): clip(v + trunc(N(mean, sigma)), 0, 65535).
 *   POISSON     apply_quantum_noise(src, factor): k ~ Poisson(v * factor), then float(k) / float(factor) in f32, clipped, truncated.
 * The noise draws come from Philox4x32-10 (Salmon et al., SC 2011): the key is (seed & 0xffffffff, seed >> 32), and block j = 0, 1, ..
 * of pixel p (its row-major index y * N + x) is the output (x, y, z, w) of the counter (p, j, stream, 0). A block yields two uniform
 * doubles in [0, 1), u53(x, y) first and then u53(z, w), with u53(a, b) = ((a >> 5) * 2^26 + (b >> 6)) / 2^53 (numpy's next_double); a
 * pixel consumes its uniforms in that order, starting at block 0 for every call. So a pixel's value depends on the spec, its source
 * value and its index only: not on N, image_index or the launch. The samplers follow numpy's distributions but not numpy's stream:
 *   normal   Box-Muller in f64 on the pixel's first two uniforms, z = sqrt(-2 ln(1 - u0)) cos(2 pi u1); the draw is mean + sigma z
 *            truncated toward zero and saturated to int32.
 *   Poisson  0 when lambda is not > 0 (no uniform consumed); below lambda = 10 the number of uniforms multiplied together, one per
 *            round, before the product is no longer > exp(-lambda), less one; from 10 on Hormann's PTRS (1993) with its constants, two
 *            uniforms per round: U = u - 0.5 first, then V.
 * tests/noise_restatement.py states this contract in numpy; the draws are compared with it pixel for pixel.
 *   SYMMETRY    element `dx` (0 .. 7) of the square's symmetry group (D4), np.rot90(src if dx < 4 else src.T, dx & 3), bit-exact: a
 *               permutation of the source, no fill and no resampling (harness.apply_symmetry). Output pixel (i, j) is source pixel
 *               0: [i, j]   1: [j, N-1-i]   2: [N-1-i, N-1-j]   3: [N-1-j, i]   4: [j, i]   5: [N-1-i, j]   6: [N-1-j, N-1-i]   7: [i, N-1-j]. */
typedef enum musica_alteration_kind {
    MUSICA_ALTER_NONE = 0,
    MUSICA_ALTER_TRANSLATE = 1,
    MUSICA_ALTER_ROTATE = 2,
    MUSICA_ALTER_COLLIMATOR = 3,
    MUSICA_ALTER_GAUSSIAN = 4,
    MUSICA_ALTER_POISSON = 5,
    MUSICA_ALTER_SYMMETRY = 6,
    MUSICA_ALTER_KIND_COUNT = 7
} musica_alteration_kind;
typedef struct musica_alteration {
    uint32_t kind;                  /* musica_alteration_kind */
    int32_t dx, dy;                 /* TRANSLATE: x_shift, y_shift (|shift| < N); SYMMETRY: dx is the element, 0 .. 7 */
    int32_t margin;                 /* ROTATE: the crop's margin, 0 <= 2 margin < N */
    int32_t shutter_h, shutter_v;   /* COLLIMATOR: 0 <= 2 shutter <= N */
    double mean, sigma;             /* GAUSSIAN: sigma finite and > 0, mean finite */
    double factor;                  /* POISSON: finite, > 0, 65535 * factor < 2^30 */
    uint64_t seed;                  /* noise kinds: the Philox key (low word, high word) */
    uint32_t stream;                /* noise kinds: word 2 of the Philox counter */
    double matrix[4];               /* ROTATE: rot_matrix of ndimage.rotate, row-major */
    double offset[2];               /* ROTATE: its offset */
} musica_alteration;
/* N x N host pixels into the source plane (allocated on first use; synchronous). */
int musica_alter_set_source(musica_ctx* ctx, const uint16_t* pixels);
/* The alteration of the source into image `image_index` of the input buffer, enqueued on the ctx stream (follow it with
 * musica_execute_device(ctx, musica_input_device_ptr(ctx))). Refused before any device work: no source, a kind out of range,
 * image_index >= batch, shifts or shutters that leave nothing, a margin that leaves no crop, a non-finite or non-positive sigma or factor,
 * a non-finite matrix or offset, a symmetry element outside 0 .. 7. It changes no other image of the input buffer, no result of the last step and no reference slot. */
int musica_alter(musica_ctx* ctx, uint32_t image_index, const musica_alteration* spec);
/* binomial_blur(source plane, radius) (above, at musica_sim_blur_reference) into image `image_index` of the input buffer, enqueued on the
 * ctx stream, with musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no reference
 * slot. An entry point of its own and not a musica_alteration_kind: the kinds are closed at MUSICA_ALTER_KIND_COUNT. Refused before any
 * device work: no source, image_index >= batch, a radius outside 1 .. MUSICA_BLUR_MAX_RADIUS. */
int musica_alter_blur(musica_ctx* ctx, uint32_t image_index, uint32_t radius);
/* block_codec(source plane, table, (0, 0)) (above, at musica_sim_codec_reference) into image `image_index` of the input buffer, enqueued
 * on the ctx stream, with musica_alter's guarantees. Refused before any device work: a NULL context, a NULL table, no source,
 * a table entry of 0, image_index >= batch. */
int musica_alter_codec(musica_ctx* ctx, uint32_t image_index, const uint16_t table[64]);
/* zoom(source plane, (p, q)) (above, at musica_sim_zoom_reference) into image `image_index` of the input buffer, enqueued on the ctx
 * stream, with musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no reference
 * slot. An entry point of its own and not a musica_alteration_kind: the kinds are closed at MUSICA_ALTER_KIND_COUNT. Refused before any
 * device work: a NULL context, no source, q = 0, p <= q, p > MUSICA_ZOOM_MAX_P, gcd(p, q) != 1, image_index >= batch. */
int musica_alter_zoom(musica_ctx* ctx, uint32_t image_index, uint32_t p, uint32_t q);
/* scatter(source plane, (radius, num, den)) (above, at musica_sim_scatter_reference) into image `image_index` of the input buffer,
 * enqueued on the ctx stream, with musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step
 * and no reference slot. An entry point of its own and not a musica_alteration_kind: the kinds are closed at MUSICA_ALTER_KIND_COUNT.
 * Refused before any device work: a NULL context, no source, a radius outside 1 .. MUSICA_SCATTER_MAX_RADIUS, num = 0, num >= den,
 * den > MUSICA_SCATTER_MAX_DEN, gcd(num, den) != 1, image_index >= batch, a failed allocation of the row plane. */
int musica_alter_scatter(musica_ctx* ctx, uint32_t image_index, uint32_t radius, uint32_t num, uint32_t den);
/* warp(source plane, field, origin (0, 0)) (above, at musica_sim_warp_reference) into image `image_index` of the input buffer, enqueued
 * on the ctx stream, with musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no
 * reference slot. An entry point of its own and not a musica_alteration_kind: the kinds are closed at MUSICA_ALTER_KIND_COUNT. `field`:
 * nodes x nodes x 2 host int16, row-major, (dx, dy) per node, borrowed for the call. Refused before any device work: a NULL context or
 * field, no source, `nodes` below ((N - 1) >> 6) + 2 or above MUSICA_WARP_MAX_NODES, a node component outside +-MUSICA_WARP_MAX_SHIFT
 * (the refusal names the node), image_index >= batch. */
int musica_alter_warp(musica_ctx* ctx, uint32_t image_index, const int16_t* field, uint32_t nodes);
/* Test hook: the N x N integer draws of a noise alteration (k of COLLIMATOR / POISSON, for every pixel; the truncated noise of GAUSSIAN),
 * the same numbers musica_alter uses. Synchronous. */
int musica_alter_draws(musica_ctx* ctx, const musica_alteration* spec, int32_t* dst);
/* np.percentile(src[y:y + h, x:x + w], q) (numpy's default 'linear' method) of the source plane, computed on the device
 * as the fills are; synchronous. */
int musica_alter_percentile(musica_ctx* ctx, uint32_t x, uint32_t y, uint32_t w, uint32_t h, double q, double* out);

/* ---- contrast-detail: inserted discs, measured where they lie (new, not in the reference) ----
 * The one relation of the study that changes the input locally and measures the output locally: does a small low-contrast object come
 * out visible, and equally so wherever it lies? harness.insert_details, harness.detail_statistics and harness.detail_summary are the
 * contract; everything is integer and the device is bit-identical to them, from call to call as well (no atomics, one reduction order).
 * A detail is (x, y, radius, contrast): an integer pixel centre, 1 <= radius <= MUSICA_DETAIL_MAX_RADIUS, 1 <= |contrast| <=
 * MUSICA_DETAIL_MAX_CONTRAST. With d2 = (px - x)^2 + (py - y)^2 its zones are
 *   disc   d2 <= r^2
 *   ring   (r + 2)^2 <= d2 <= (2r + 2)^2
 *   box    |px - x| <= 2r + 2 and |py - y| <= 2r + 2       (side 4r + 5)
 * A list for a plane of side n holds 1 .. MUSICA_DETAIL_MAX details whose boxes lie inside [0, n)^2 and are pairwise disjoint
 * (|xi - xj| > Roi + Roj or |yi - yj| > Roi + Roj with Ro = 2r + 2): a pixel belongs to at most one disc, so nothing depends on the
 * list's order. Both entry points refuse every other list before any device work.
 *   insertion   inside a disc out = min((v * (1024 - contrast) + 512) >> 10, 65535), every other pixel copied. contrast > 0 attenuates
 *               as an absorbing object does, contrast < 0 brightens as a void does; ONE rounding, halves up; the largest intermediate is
 *               65535 * 1536 + 512 < 2^32. With |contrast| <= 512 a non-zero pixel stays non-zero (v >= 1 gives (512 + 512) >> 10 = 1),
 *               so an insertion never creates the zeros that the noise and gradation histograms treat specially.
 *   statistics  per detail and for the disc and the ring: the pixel count n and the sums of a, b, a^2, b^2 and a b over the zone; over
 *               the box the sum of (a - b)^2 and its pixel count (4r + 5)^2. `contrast` is not looked at.
 * The attenuation is defined on detector counts, not on the graded 8-bit plane: there is no musica_sim_..._reference sibling that
 * would insert details into a reference slot. */
#define MUSICA_DETAIL_MAX_RADIUS 64
#define MUSICA_DETAIL_MAX_CONTRAST 512
#define MUSICA_DETAIL_MAX 1024
typedef struct musica_detail {
    int32_t x, y;                   /* the centre, in pixels of the plane the call names */
    uint32_t radius;                /* 1 .. MUSICA_DETAIL_MAX_RADIUS */
    int32_t contrast;               /* 1 <= |contrast| <= MUSICA_DETAIL_MAX_CONTRAST, in 1 / 1024 of the pixel's value */
} musica_detail;
typedef struct musica_sim_detail_result {   /* index 0: the disc, index 1: the ring */
    uint64_t n[2];                  /* pixels of the zone */
    uint64_t sum_a[2], sum_b[2];    /* sums over the zone of side a (the output) and side b (the slot) */
    uint64_t sum_aa[2], sum_bb[2], sum_ab[2];
    uint64_t box_ssd;               /* sum over the box of (a - b)^2 */
    uint64_t box_pixels;            /* (4 radius + 5)^2 */
} musica_sim_detail_result;
/* insert_details(source plane, details) into image `image_index` of the input buffer: the details are in the N x N plane's
 * coordinates. The kernel is enqueued on the ctx stream (the list is copied to the device first, which waits for what the stream
 * holds), with musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no reference
 * slot. One launch, 2 bytes read and 2 written per pixel (kernels_details.hip). Refused before any device work: a NULL context or list,
 * no source, image_index >= batch, a count outside 1 .. MUSICA_DETAIL_MAX, a radius or contrast outside its limits, a box that leaves
 * the plane, two boxes that are not disjoint. */
int musica_alter_details(musica_ctx* ctx, uint32_t image_index, uint32_t count, const musica_detail* details);
/* detail_statistics of side a, the 8-bit output of batch image `image_index` (quantised while read, exactly as musica_sim_compare
 * reads it), against side b, reference slot `slot`: results[i] for details[i], in the coordinates of the (N - 20)^2 output plane.
 * Synchronous. box_ssd equals musica_sim_compare's sq_diff_sum over the same (4r + 5)^2 region. Refused before any device work: a NULL
 * context, list or results, a count outside 1 .. MUSICA_DETAIL_MAX, an image too small for the margin, a slot out of range or never
 * written, image_index >= batch, a radius outside its limits, a box that leaves the plane, two boxes that are not disjoint. */
int musica_sim_details(musica_ctx* ctx, uint32_t image_index, uint32_t slot, uint32_t count, const musica_detail* details,
                       musica_sim_detail_result* results);

/* ---- edge response: slanted edges, the edge-spread function binned where they lie (new, not in the reference) ----
 * How does the processor render an edge: the edge-spread function, its overshoot and undershoot (the rebound halo of multi-scale
 * amplifiers), the 10-90 % rise and the edge MTF, and do they depend on the edge's contrast, position, orientation and polarity? The
 * ISO 12233 / IEC 62220 slanted edge with a rational slope of our choosing. harness.insert_edges, harness.edge_statistics and
 * harness.edge_summary are the contract; everything the device computes is integer and bit-identical to them, from call to call as
 * well (integer LDS atomics and one reduction order).
 * An edge is (x, y, half, p, q, orientation, contrast): an integer pixel centre, MUSICA_EDGE_MIN_HALF <= half <= MUSICA_EDGE_MAX_HALF,
 * the slope p / q with 1 <= p < q, MUSICA_EDGE_MIN_Q <= q <= MUSICA_EDGE_MAX_Q and gcd(p, q) = 1, orientation 0 .. 3 and
 * 1 <= |contrast| <= MUSICA_EDGE_MAX_CONTRAST in 1 / 1024 of the pixel's value. With dx = px - x, dy = py - y the profile coordinate u
 * and the along-edge coordinate v are (dx, dy), (dy, dx), (-dx, dy), (-dy, dx) for orientation 0, 1, 2, 3, and the signed numerator is
 * s = q u - p v. Zones:
 *   plate    |dx|, |dy| <= 2 half     (side 4 half + 1): what gets inserted
 *   region   |dx|, |dy| <= half       (side 2 half + 1): what gets measured
 * A list for a plane of side n holds 1 .. MUSICA_EDGE_MAX edges whose plates lie inside [0, n)^2 and are pairwise disjoint
 * (|xi - xj| > 2 (hi + hj) or |yi - yj| > 2 (hi + hj)): a pixel belongs to at most one plate, so nothing depends on the list's
 * order. Both entry points refuse every other list before any device work.
 *   insertion   inside a plate, with m = clamp(2s + q, 0, 2q): out = min((v * (2048 q - contrast * m) + 1024 q) div (2048 q), 65535),
 *               every other pixel copied. m / 2q is the part of the pixel's one-pixel box aperture along the profile axis that the
 *               absorber covers; ONE rounding, halves up; m = 0 gives v, m = 2q the detail's min((v * (1024 - contrast) + 512) >> 10,
 *               65535); the largest intermediate is 65535 * (2048 * 16 + 512 * 32) + 16384 < 2^32.
 *   statistics  per edge a table of 2B + 1 bins, B = ceil(4 (q + p) half / q) (musica_edge_bins; at most 2047): every pixel of the
 *               region falls in bin k = floor(4 s / q), stored at index k + B, and each bin holds the exact n, sum_a, sum_b and
 *               sum_aa of its pixels (at most 2 half + 1 of them: every sum fits uint32); and over the region the sum of (a - b)^2
 *               and its pixel count. `contrast` is not looked at.
 * As for the details there is no musica_sim_..._reference sibling. */
#define MUSICA_EDGE_MIN_HALF 8
#define MUSICA_EDGE_MAX_HALF 128
#define MUSICA_EDGE_MIN_Q 4
#define MUSICA_EDGE_MAX_Q 16
#define MUSICA_EDGE_MAX_CONTRAST 512
#define MUSICA_EDGE_MAX 256
#define MUSICA_EDGE_BINS_MAX 2048
typedef struct musica_edge {
    int32_t x, y;                   /* the centre, in pixels of the plane the call names */
    uint32_t half;                  /* MUSICA_EDGE_MIN_HALF .. MUSICA_EDGE_MAX_HALF */
    uint32_t p, q;                  /* the slope p / q: 1 <= p < q, MUSICA_EDGE_MIN_Q <= q <= MUSICA_EDGE_MAX_Q, lowest terms */
    uint32_t orientation;           /* 0 .. 3 */
    int32_t contrast;               /* 1 <= |contrast| <= MUSICA_EDGE_MAX_CONTRAST, in 1 / 1024 of the pixel's value */
} musica_edge;
typedef struct musica_sim_edge_result {
    uint64_t roi_ssd;               /* sum over the region of (a - b)^2 */
    uint64_t roi_pixels;            /* (2 half + 1)^2 */
    uint64_t table_offset;          /* where the edge's table starts in `tables`, in words: 4 times the bins of the edges before it */
    uint64_t bins;                  /* 2B + 1 */
} musica_sim_edge_result;
/* The bins 2B + 1 of the table of an edge of this half-side and slope, or 0 for an inadmissible triple. No context, no device. */
uint32_t musica_edge_bins(uint32_t half, uint32_t p, uint32_t q);
/* insert_edges(source plane, edges) into image `image_index` of the input buffer: the edges are in the N x N plane's coordinates. The
 * kernel is enqueued on the ctx stream (the list is copied to the device first, which waits for what the stream holds), with
 * musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no reference slot. One
 * launch, 2 bytes read and 2 written per pixel (kernels_edges.hip). Refused before any device work: a NULL context or list, no source,
 * image_index >= batch, a count outside 1 .. MUSICA_EDGE_MAX, a half-side, slope, orientation or contrast outside its limits, a plate
 * that leaves the plane, two plates that are not disjoint. */
int musica_alter_edges(musica_ctx* ctx, uint32_t image_index, uint32_t count, const musica_edge* edges);
/* edge_statistics of side a, the 8-bit output of batch image `image_index` (quantised while read, exactly as musica_sim_compare reads
 * it), against side b, reference slot `slot`: results[i] for edges[i], in the coordinates of the (N - 20)^2 output plane. `tables` is
 * flat: edge i starts at the sum over j < i of 4 * bins_j words (results[i].table_offset) and is laid out [4][bins_i]: n, sum_a, sum_b,
 * sum_aa; table_words, the words `tables` has room for, must be at least the total. Synchronous. roi_ssd equals musica_sim_compare's
 * sq_diff_sum over the same (2 half + 1)^2 region. Refused before any device work: a NULL context, list, results or tables, a count
 * outside 1 .. MUSICA_EDGE_MAX, an image too small for the margin, a slot out of range or never written, image_index >= batch, a
 * half-side, slope or orientation outside its limits, a plate that leaves the plane, two plates that are not disjoint, table_words
 * too small. */
int musica_sim_edges(musica_ctx* ctx, uint32_t image_index, uint32_t slot, uint32_t count, const musica_edge* edges,
                     musica_sim_edge_result* results, uint32_t* tables, uint64_t table_words);

/* ---- grating response: sine patches, the region folded by phase where they lie (new, not in the reference) ----
 * What defines a multi-scale contrast equaliser: its gain as a function of spatial frequency AND of amplitude, and the harmonic
 * distortion of a pure tone, the direct signature of the non-linearity. The line-pair / sine grating patch. harness.insert_gratings,
 * harness.grating_statistics and harness.grating_summary are the contract; everything the device computes is integer and
 * bit-identical to them, from call to call as well (integer LDS atomics and one reduction order).
 * A grating is (x, y, half, ux, uy, period) and a wave table: an integer pixel centre, MUSICA_GRATING_MIN_HALF <= half <=
 * MUSICA_GRATING_MAX_HALF, the wave vector (ux, uy) with |ux|, |uy| <= MUSICA_GRATING_MAX_U, not both 0, gcd(|ux|, |uy|) = 1, and the
 * period T with 2 <= T <= MUSICA_GRATING_MAX_PERIOD, T <= half, 2 |ux| <= T and 2 |uy| <= T (no aliasing along either axis): |u| / T
 * cycles per pixel along u. With dx = px - x, dy = py - y the phase of a pixel is k = (ux dx + uy dy) mod T, in 0 .. T - 1. The wave
 * is T integers in 1 / 1024 of the pixel's value, |w| <= MUSICA_GRATING_MAX_CONTRAST. Zones, as for the edges:
 *   plate    |dx|, |dy| <= 2 half     (side 4 half + 1): what gets inserted
 *   region   |dx|, |dy| <= half       (side 2 half + 1): what gets measured
 * A list for a plane of side n holds 1 .. MUSICA_GRATING_MAX gratings whose plates lie inside [0, n)^2 and are pairwise disjoint
 * (|xi - xj| > 2 (hi + hj) or |yi - yj| > 2 (hi + hj)): a pixel belongs to at most one plate, so nothing depends on the list's
 * order. The waves travel in one flat array, grating i's table at the sum of the periods before it. Both entry points refuse every
 * other list before any device work.
 *   insertion   inside a plate out = min((v * (1024 - wave[k]) + 512) >> 10, 65535), every other pixel copied. ONE rounding, halves
 *               up; wave[k] = 0 gives v exactly; the largest intermediate is 65535 * 1536 + 512 < 2^32; a non-zero pixel stays
 *               non-zero.
 *   statistics  per grating a table of T bins: every pixel of the region falls in bin k, and each bin holds the exact n, sum_a, sum_b
 *               and sum_aa of its pixels; and over the region the sum of (a - b)^2 and its pixel count. The wave is not looked at.
 *               Every bin is non-empty (dx and dy each run over at least T consecutive values and reach the multiples of gcd(ux, T)
 *               and of gcd(uy, T), together those of gcd(ux, uy, T) = 1). A bin holds at most ceil(S / 2) S pixels, S = 2 half + 1
 *               <= 257 (one of ux, uy is not 0 mod T, so along that axis a phase repeats at a period of at least 2): 33153 pixels,
 *               33153 * 255^2 < 2^32, every sum fits uint32.
 * As for the details and the edges there is no musica_sim_..._reference sibling. */
#define MUSICA_GRATING_MIN_HALF 8
#define MUSICA_GRATING_MAX_HALF 128
#define MUSICA_GRATING_MAX_U 8
#define MUSICA_GRATING_MAX_PERIOD 64
#define MUSICA_GRATING_MAX_CONTRAST 512
#define MUSICA_GRATING_MAX 256
typedef struct musica_grating {
    int32_t x, y;                   /* the centre, in pixels of the plane the call names */
    uint32_t half;                  /* MUSICA_GRATING_MIN_HALF .. MUSICA_GRATING_MAX_HALF */
    int32_t ux, uy;                 /* the wave vector: |ux|, |uy| <= MUSICA_GRATING_MAX_U, not both 0, coprime */
    uint32_t period;                /* T: 2 .. MUSICA_GRATING_MAX_PERIOD, T <= half, 2 |ux| <= T, 2 |uy| <= T */
} musica_grating;
typedef struct musica_sim_grating_result {
    uint64_t roi_ssd;               /* sum over the region of (a - b)^2 */
    uint64_t roi_pixels;            /* (2 half + 1)^2 */
    uint64_t table_offset;          /* where the grating's table starts in `tables`, in words: 4 times the periods of the gratings before it */
    uint64_t bins;                  /* T */
} musica_sim_grating_result;
/* insert_gratings(source plane, gratings) into image `image_index` of the input buffer: the gratings are in the N x N plane's
 * coordinates, `waves` holds wave_words int16, grating i's `period` entries at the sum of the periods before it. The kernel is
 * enqueued on the ctx stream (the list and the waves are copied to the device first, which waits for what the stream holds), with
 * musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no reference slot. One
 * launch, 2 bytes read and 2 written per pixel (kernels_gratings.hip). Refused before any device work: a NULL context, list or waves,
 * no source, image_index >= batch, a count outside 1 .. MUSICA_GRATING_MAX, a half-side, wave vector or period outside its limits, a
 * plate that leaves the plane, two plates that are not disjoint, wave_words less than the periods' sum, a wave entry beyond
 * +- MUSICA_GRATING_MAX_CONTRAST. */
int musica_alter_gratings(musica_ctx* ctx, uint32_t image_index, uint32_t count, const musica_grating* gratings, const int16_t* waves,
                          uint64_t wave_words);
/* grating_statistics of side a, the 8-bit output of batch image `image_index` (quantised while read, exactly as musica_sim_compare
 * reads it), against side b, reference slot `slot`: results[i] for gratings[i], in the coordinates of the (N - 20)^2 output plane.
 * `tables` is flat: grating i starts at 4 times the sum over j < i of period_j words (results[i].table_offset) and is laid out
 * [4][period_i]: n, sum_a, sum_b, sum_aa; table_words, the words `tables` has room for, must be at least the total. Synchronous.
 * roi_ssd equals musica_sim_compare's sq_diff_sum over the same (2 half + 1)^2 region. Refused before any device work: a NULL context,
 * list, results or tables, a count outside 1 .. MUSICA_GRATING_MAX, an image too small for the margin, a slot out of range or never
 * written, image_index >= batch, a half-side, wave vector or period outside its limits, a plate that leaves the plane, two plates
 * that are not disjoint, table_words too small. */
int musica_sim_gratings(musica_ctx* ctx, uint32_t image_index, uint32_t slot, uint32_t count, const musica_grating* gratings,
                        musica_sim_grating_result* results, uint32_t* tables, uint64_t table_words);

/* ---- detector gain: a separable gain map, and the row and column profiles of a comparison (new, not in the reference) ----
 * What varies first from one exposure to the next is the detector's gain: the dose (one constant), the heel effect and vignetting
 * (smooth multiplicative shading), the gain error of a readout block and the single uncorrected column or row. One separable map
 * covers them, out(x, y) = v gx[x] gy[y], and one measurement scores them: the exact profiles of a comparison along both axes, where a
 * line artefact far below the pixel noise shows because a profile integrates along it. harness.apply_gain and
 * harness.profile_statistics are the contract; everything the device computes is integer and bit-identical to them, from call to call
 * as well.
 * A gain map is two tables of N uint16_t for the N x N raw plane, gx per column and gy per row, in units of 1 / MUSICA_GAIN_ONE. Every
 * value 0 .. 65535 is allowed: 0 is a dead line, 65535 about 16 x.
 *   g   = gx[x] * gy[y]                          fits uint32: 65535^2 < 2^32
 *   out = min((v * g + 2^23) >> 24, 65535)       ONE rounding, halves up; the largest intermediate is 65535^3 + 2^23 < 2^48
 * gx = gy = MUSICA_GAIN_ONE returns v exactly (v * 2^24 + 2^23 >> 24 = v). The clamp at 65535 is the detector's saturation and part of
 * the contract. There is no musica_sim_gain_reference sibling: what a normalising processor is expected to show is invariance, which the
 * direct comparison scores. */
#define MUSICA_GAIN_ONE 4096
/* apply_gain(source plane, gx, gy) into image `image_index` of the input buffer: gx and gy hold N host values each. The kernel is
 * enqueued on the ctx stream (the tables are copied to the device first, which waits for what the stream holds), with musica_alter's
 * guarantees: it changes no other image of the input buffer, no result of the last step and no reference slot. One launch, 2 bytes read
 * and 2 written per pixel (kernels_gain.hip). An entry point of its own and not a musica_alteration_kind: the kinds are closed at
 * MUSICA_ALTER_KIND_COUNT. Refused before any device work: a NULL context or table, no source, image_index >= batch. */
int musica_alter_gain(musica_ctx* ctx, uint32_t image_index, const uint16_t* gx, const uint16_t* gy);
/* The profiles of `count` (1 .. MUSICA_PROFILE_MAX_QUERIES) comparisons in one launch. A query is musica_sim_compare's: side a the 8-bit
 * output of batch image `image_index` (quantised while read, exactly as musica_sim_compare reads it), side b reference slot `slot`, the
 * region (ax, ay) / (bx, by), w x h with w, h >= 1. Query i gets a column table [w][4] followed by a row table [h][4] in the flat
 * `tables`, from results[i].table_offset (in words: the sum over j < i of 4 (w_j + h_j)) on. A line's four words are the exact
 *   sum_a, sum_b, sum_dd = sum of (a - b)^2, sum_aa
 * over the line's pixels inside the region: h pixels for a column, w for a row. A line has at most 16364 pixels (N <= 16384) and
 * 16364 * 255^2 < 2^32, so everything fits uint32. results[i].ssd is the sum of either table's sum_dd and equals musica_sim_compare's
 * sq_diff_sum over the same region. table_words, the words `tables` has room for, must be at least the total. Synchronous; integers
 * only, byte-identical from call to call. Refused before any device work: what musica_sim_compare refuses, except that the smallest
 * side is 1 and the largest count MUSICA_PROFILE_MAX_QUERIES, a NULL `tables`, and table_words too small. */
#define MUSICA_PROFILE_MAX_QUERIES 16
typedef struct musica_sim_profile_result {
    uint64_t table_offset;          /* where the query's column table starts in `tables`, in words; its row table follows at + 4 cols */
    uint64_t cols, rows;            /* w, h */
    uint64_t ssd;                   /* sum over the region of (a - b)^2 */
    uint64_t pixels;                /* w * h */
} musica_sim_profile_result;
int musica_sim_profiles(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_profile_result* results,
                        uint32_t* tables, uint64_t table_words);

/* ---- tone tables: a point-wise map of the input's gray levels, and the output per input level (new, not in the reference) ----
 * Every other alteration moves, blurs, shades or adds to the input; none changes its gray levels point-wise: a dark-current pedestal,
 * a non-linear detector characteristic, a coarser ADC, saturation, a negative. That is the axis on which MUSICA promises most (sqrt,
 * min, max and normalise in front, a tone curve built from the image's own histogram behind). One table covers them, out = lut[v], and
 * one measurement scores them: the exact sums of a comparison kept apart by the level of the INPUT pixel, which give the chain's
 * characteristic curve (mean output per input level) before and after, and split the change of the output into a part that is a
 * function of the input level alone and a remainder. harness.apply_lut and harness.level_statistics are the contract; everything the
 * device computes is integer and bit-identical to them, from call to call as well.
 * A table holds MUSICA_LUT_ENTRIES uint16_t, one for every value a raw pixel can take; every table is allowed. The identity copies. */
#define MUSICA_LUT_ENTRIES 65536
/* apply_lut(source plane, lut) into image `image_index` of the input buffer: lut holds MUSICA_LUT_ENTRIES host values. The kernel is
 * enqueued on the ctx stream (the table is copied to a context-owned 128 KiB device buffer first, allocated on first use, which waits
 * for what the stream holds), with musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step
 * and no reference slot. One launch, 2 bytes read and 2 written per pixel, the table staged in LDS (kernels_levels.hip). An
 * entry point of its own and not a musica_alteration_kind: the kinds are closed at MUSICA_ALTER_KIND_COUNT. Refused before any device
 * work: a NULL context or table, no source, image_index >= batch. */
int musica_alter_lut(musica_ctx* ctx, uint32_t image_index, const uint16_t* lut);
/* The levels of `count` (1 .. MUSICA_LEVEL_MAX_QUERIES) comparisons in one launch. A query is musica_sim_compare's: side a the 8-bit
 * output of batch image `image_index` (quantised while read, exactly as musica_sim_compare reads it), side b reference slot `slot`, the
 * region (ax, ay) / (bx, by), w x h with w, h >= 1. The class of a-side pixel (x, y) of the output plane is
 *   source[(y + MUSICA_OUT_MARGIN) * N + x + MUSICA_OUT_MARGIN] >> shift
 * with the alteration source plane (musica_alter_set_source) and shift in MUSICA_LEVEL_MIN_SHIFT .. MUSICA_LEVEL_MAX_SHIFT, so there
 * are C = (65535 >> shift) + 1 <= 4096 classes: the level of the unaltered input under the pixel, whatever origin side b has. Query i
 * gets a table [C][MUSICA_LEVEL_WORDS] of uint64_t in the flat `tables`, from results[i].table_offset (in words: i * C *
 * MUSICA_LEVEL_WORDS) on. A class's six words are the exact
 *   n, sum_a, sum_b, sum_dd = sum of (a - b)^2, sum_aa, sum_bb
 * over the region's pixels of that class. The n of a table add up to w * h and results[i].ssd, the sum of its sum_dd, equals
 * musica_sim_compare's sq_diff_sum over the same region. table_words, the words `tables` has room for, must be at least count * C *
 * MUSICA_LEVEL_WORDS. Synchronous; integers only, byte-identical from call to call. Refused before any device work: what
 * musica_sim_compare refuses, except that the smallest side is 1 and the largest count MUSICA_LEVEL_MAX_QUERIES, then no source plane,
 * a shift out of range, a NULL `tables`, and table_words too small. After a refusal the context stays usable. */
#define MUSICA_LEVEL_MAX_QUERIES 4
#define MUSICA_LEVEL_MIN_SHIFT 4
#define MUSICA_LEVEL_MAX_SHIFT 15
#define MUSICA_LEVEL_WORDS 6
typedef struct musica_sim_level_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t classes;               /* C */
    uint64_t ssd;                   /* sum over the region of (a - b)^2 */
    uint64_t pixels;                /* w * h */
} musica_sim_level_result;
int musica_sim_levels(musica_ctx* ctx, uint32_t shift, uint32_t count, const musica_sim_query* queries, musica_sim_level_result* results,
                      uint64_t* tables, uint64_t table_words);

/* ---- gradient metrics: the Sobel gradients of a comparison, by the edge strength of the reference (new, not in the reference) ----
 * MUSICA amplifies weak gradients more than strong ones; every other measurement compares gray levels, windows, scales, positions, lines
 * or planted patches. This one compares the edges of the image itself. metrics.gradient_statistics is the contract; every word of the
 * tables is an exact integer equal to it and byte-identical from call to call.
 * A query is musica_sim_compare's (side a the 8-bit output of batch image `image_index`, quantised while read exactly as
 * musica_sim_compare reads it; side b reference slot `slot`; w, h >= 7). Over the INTERIOR of the region, the (w - 2) x (h - 2) pixels
 * whose 3 x 3 neighbourhood lies inside the region (no pixel outside a region is read), both sides get the integer Sobel gradient
 *   gx = (p[y-1][x+1] + 2 p[y][x+1] + p[y+1][x+1]) - (the same at x - 1)
 *   gy = (p[y+1][x-1] + 2 p[y+1][x] + p[y+1][x+1]) - (the same at y - 1)
 * both in -1020 .. 1020, and per pixel the terms
 *   A = gxa^2 + gya^2, B = gxb^2 + gyb^2, dot = gxa gxb + gya gyb, cross = gxa gyb - gya gxb
 * each of magnitude <= 1 300 500 (attained by A and B at the neighbourhood [[0,0,255],[0,.,255],[0,255,255]]). A pixel's class is the
 * bit length of B, 0 .. 21: class 0 is a reference pixel without gradient, class 21 starts at 2^20 (a diagonal step, gx = gy = 765).
 * Query i gets a table [MUSICA_GRADIENT_CLASSES][MUSICA_GRADIENT_WORDS] of uint64_t in the flat `tables`, from
 * results[i].table_offset (in words: i * MUSICA_GRADIENT_CLASSES * MUSICA_GRADIENT_WORDS) on. A class's six words are
 *   n, sum A, sum B, sum dot, sum cross, neg = the number of its pixels with dot < 0
 * sum dot and sum cross signed, in two's complement. The n of a table add up to results[i].pixels = (w - 2) (h - 2).
 * results[i].gsim is the mean over the interior of q = (2 dot + C) / (A + B + C), C = MUSICA_GRADIENT_C = 2720 (the 170 of GMSD, Xue et
 * al. 2014, stated for Prewitt / 3, carried to Sobel's squared scale: x 16): numerator and denominator exact integers below 2^53, one
 * correctly rounded f64 division per pixel, the sum in the device's own FIXED order (per-workgroup partials folded by a second launch,
 * no f64 atomics), so it repeats bit for bit and agrees with the host's math.fsum within rounding; identical sides give exactly 1.0.
 * Every word of the count tables is written and nothing behind them. Synchronous, on the context's stream after whatever was enqueued
 * there; changes no slot, no result of a step and no input image; scratch is allocated on first use. Refused before any device work:
 * what musica_sim_compare refuses, then a NULL `tables` and table_words < count * MUSICA_GRADIENT_CLASSES * MUSICA_GRADIENT_WORDS.
 * After a refusal the context stays usable. */
#define MUSICA_GRADIENT_CLASSES 22
#define MUSICA_GRADIENT_WORDS 6
#define MUSICA_GRADIENT_C 2720
typedef struct musica_sim_gradient_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t pixels;                /* (w - 2) * (h - 2) */
    double gsim;                    /* mean of q over the interior */
} musica_sim_gradient_result;
int musica_sim_gradients(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_gradient_result* results,
                         uint64_t* tables, uint64_t table_words);

/* ---- local order: the census signs of a comparison (new, not in the reference) ----
 * MUSICA ends in a monotone tone curve, and most alterations move gray levels without changing the scene. Every other measurement
 * charges the values that moved; this one asks whether the same pixel is still the darker one of a neighbouring pair (the census
 * transform, Zabih & Woodfill 1994). metrics.order_statistics is the contract; every word of the tables is an exact integer equal to it
 * and byte-identical from call to call. There is no float on the device: every derived number is the host's (metrics.order_summary).
 * A query is musica_sim_compare's (side a the 8-bit output of batch image `image_index`, quantised while read exactly as
 * musica_sim_compare reads it; side b reference slot `slot`; w, h >= 7). Over the INTERIOR of the region, the (w - 6) x (h - 6) pixels
 * whose 7 x 7 neighbourhood lies inside the region (no pixel outside a region is read), a pixel c and each of its 48 neighbours n give
 * one sign per side, s = sign(p[n] - p[c]) in {-1, 0, +1}, in the ring max(|dx|, |dy|) = 1, 2, 3 of 8, 16 and 24 neighbours. A (pixel,
 * neighbour) pair is
 *   same       sa = sb != 0      the order is kept
 *   reversed   sa = -sb != 0     the order is reversed
 *   flattened  sa = 0, sb != 0   the output ties where the reference orders
 *   split      sa != 0, sb = 0   the output orders where the reference ties
 * or tied on both sides. The census distance of a pixel is d = sum |sa - sb| over its 48 neighbours = 2 reversed + flattened + split,
 * 0 .. 96. Query i gets MUSICA_ORDER_TABLE_WORDS uint64_t in the flat `tables`, from results[i].table_offset (in words: i *
 * MUSICA_ORDER_TABLE_WORDS) on: first [MUSICA_ORDER_RINGS][MUSICA_ORDER_WORDS], per ring
 *   pairs (results[i].pixels x 8, 16, 24), same, reversed, flattened, split          (the pairs tied on both sides are the remainder)
 * then [MUSICA_ORDER_BINS], the number of interior pixels at each d; they add up to results[i].pixels = (w - 6) (h - 6), and
 * sum d hist[d] equals the rings' sum of 2 reversed + flattened + split. Only ring sums are shown, so the order of the neighbours
 * inside a ring is the implementation's own. Identical sides give reversed = flattened = split = 0 and hist[0] = pixels; swapping the
 * sides swaps flattened and split; b -> 255 - b swaps same and reversed; a strictly increasing map of either side changes no word.
 * Every word of the tables is written and nothing behind them. Synchronous, on the context's stream after whatever was enqueued there;
 * changes no slot, no result of a step and no input image; scratch is allocated on first use. Refused before any device work: what
 * musica_sim_compare refuses, then a NULL `tables` and table_words < count * MUSICA_ORDER_TABLE_WORDS. After a refusal the context
 * stays usable. */
#define MUSICA_ORDER_RINGS 3
#define MUSICA_ORDER_WORDS 5
#define MUSICA_ORDER_BINS 97
#define MUSICA_ORDER_TABLE_WORDS 112
typedef struct musica_sim_order_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t pixels;                /* (w - 6) * (h - 6) */
} musica_sim_order_result;
int musica_sim_order(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_order_result* results,
                     uint64_t* tables, uint64_t table_words);

/* ---- lattice sums: a comparison folded by the position modulo a period (new, not in the reference) ----
 * Blocking is a lattice artefact, and so is the shift variance of a decimated pyramid, with periods 2, 4 .. 32 on the raw grid.
 * metrics.lattice_statistics is the contract. Queries are musica_sim_compare's with w, h >= 2, at most MUSICA_LATTICE_MAX_QUERIES;
 * `period` P is one of 2, 4, 8, 16, 32 and `origin` o is 0 .. P - 1. The sums run over the query's pixels (i, j) with i < w - 1 and
 * j < h - 1, so that every counted pixel has a right and a lower neighbour inside the region. The class of a pixel is
 * [(ay + j + o) mod P][(ax + i + o) mod P]: side a's position on the raw grid when o is the margin mod P. Query i gets
 * P * P * MUSICA_LATTICE_WORDS uint64_t in the flat `tables`, from results[i].table_offset (in words) on, [row phase][column phase]:
 *   n, sum a, sum b, sum (a - b)^2, sum (a[i + 1] - a[i])^2, the same of b, sum (a[j + 1] - a[j])^2, the same of b
 * The n add up to results[i].pixels = (w - 1) (h - 1); sum (a - b)^2 adds up to musica_sim_compare's sq_diff_sum of the query shrunk by
 * one column and one row; the table folded by phase mod P / 2 is the table of period P / 2 with origin o mod P / 2. Everything is an
 * integer: the tables equal the restatement word for word and repeat from call to call. Every word of the tables is written and nothing
 * behind them. Synchronous, on the context's stream after whatever was enqueued there; changes no slot, no result of a step and no input
 * image; scratch is allocated on first use. Refused before any device work: what musica_sim_compare refuses (with the smallest side 2),
 * then a period that is not one of the five, origin >= period, a NULL `tables` and table_words below the tables' words. After a
 * refusal the context stays usable. */
#define MUSICA_LATTICE_WORDS 8
#define MUSICA_LATTICE_MAX_PERIOD 32
#define MUSICA_LATTICE_MAX_QUERIES 16
typedef struct musica_sim_lattice_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t pixels;                /* (w - 1) * (h - 1) */
} musica_sim_lattice_result;
int musica_sim_lattice(musica_ctx* ctx, uint32_t period, uint32_t origin, uint32_t count, const musica_sim_query* queries,
                       musica_sim_lattice_result* results, uint64_t* tables, uint64_t table_words);

/* ---- blobs: the connected components of a comparison's change mask (new, not in the reference) ----
 * Every other measurement sums a comparison over a set chosen before the pixels are looked at; this one asks whether the changed pixels
 * form objects: scattered single-pixel flips against halos, seams, rings and blocks. metrics.blob_statistics is the contract. Queries
 * are musica_sim_compare's with w, h >= 1, at most MUSICA_BLOBS_MAX_QUERIES (a row's direct, registered and two vendor comparisons).
 * The mask of a query is |a - b| > threshold (0 .. 254) over its w x h pixels; two mask pixels are connected when they are neighbours
 * (connectivity 4: in a row or a column; 8: diagonally too), through pixels of the region only. The label of a component is 1 + the
 * row-major index y w + x, within the region, of its first pixel; 0 off the mask. Query i gets MUSICA_BLOB_CLASSES * MUSICA_BLOB_WORDS
 * uint64_t in the flat `tables`, from results[i].table_offset (in words) on; the class of a component of n pixels is
 * bit_length(n) - 1 (class 0: single pixels, class 1: 2 .. 3, ..), and per class
 *   components, pixels, sum |a - b|, sum (a - b)^2, the sum of the bounding boxes' areas, components with a pixel on the region's outline
 * The classes' pixels add up to `changed`, their components to `components`; at threshold 0 their sum (a - b)^2 adds up to
 * musica_sim_compare's sq_diff_sum. Of components of equal size the one with the smaller first pixel is the largest; where nothing
 * changed every largest_* is 0. `labels` may be NULL; else query i's plane of w h uint32_t labels, dense, starts at
 * results[i].label_offset (in words; the planes lie one behind the other). Everything is an integer and the partition is unique: the
 * results equal the restatement word for word and repeat from call to call. Every word of the tables and of the label planes is written
 * and nothing behind them. Synchronous, on the context's stream after whatever was enqueued there; changes no slot, no result of a step
 * and no input image; scratch is allocated on first use and regrown when a call needs more. Refused before any device work: what
 * musica_sim_compare refuses (with the smallest side 1), then threshold > 254, a connectivity that is neither 4 nor 8, label_words below
 * the planes' words where `labels` is given, a NULL `tables` and table_words below the tables' words. A labelling loop that reached its
 * cap (more steps than the region has pixels: a defect, never the data) is reported as "musica_sim_blobs: internal: ..." after the call
 * has run. After a refusal the context stays usable. */
#define MUSICA_BLOB_CLASSES 32
#define MUSICA_BLOB_WORDS 6
#define MUSICA_BLOBS_MAX_QUERIES 4
typedef struct musica_sim_blobs_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t label_offset;          /* where its label plane starts in `labels`, in words (whether or not labels are asked for) */
    uint64_t pixels;                /* w * h */
    uint64_t changed;               /* the mask's pixels */
    uint64_t components;
    uint64_t largest_sum_dd;        /* the largest component's sum (a - b)^2 */
    uint32_t largest_n;             /* ... its pixels */
    uint32_t largest_first;         /* ... its first pixel's row-major index in the region */
    uint32_t largest_x0, largest_y0, largest_x1, largest_y1;   /* ... its bounding box, inclusive, in the region */
} musica_sim_blobs_result;
int musica_sim_blobs(musica_ctx* ctx, uint32_t threshold, uint32_t connectivity, uint32_t count, const musica_sim_query* queries,
                     musica_sim_blobs_result* results, uint64_t* tables, uint64_t table_words, uint32_t* labels, uint64_t label_words);

/* ---- spectrum: the exact Walsh transforms of a comparison (new, not in the reference) ----
 * MUSICA amplifies bands, so its transfer function is a gain per band; this measurement takes it from the image itself: which spatial
 * frequency band and orientation was changed, and by what gain. A Fourier transform cannot be exact; the Walsh-Hadamard transform can,
 * and its octave bands are the Haar subbands. metrics.spectrum_statistics is the contract. Queries are musica_sim_compare's with
 * w, h >= 1, at most MUSICA_SPECTRUM_MAX_QUERIES (a row's direct, registered and two vendor comparisons); `tile` T is one of 8, 16, 32,
 * 64. A region holds (w / T) x (h / T) whole tiles of T x T pixels, anchored at its first pixel on either side; the remainder columns
 * and rows are not counted. W is the T x T Walsh matrix in sequency order: row s is the row of the Sylvester Hadamard matrix with exactly
 * s sign changes. Per tile A = W a W^T and B = W b W^T in integers, |A|, |B| <= 255 T^2 < 2^20. Query i gets
 * T * T * MUSICA_SPECTRUM_WORDS int64_t in the flat `tables`, from results[i].table_offset (in words) on, indexed [sv][su] with the row
 * sequency first, and per coefficient, over the region's tiles,
 *   sum A^2, sum B^2, sum A B (signed)
 * results[i].tiles = (w / T) (h / T) may be 0; the table is then all zeros. Three identities tie the table to the pixels:
 *   1. Parseval: the sum A^2 of the whole table is T^2 sum a^2 over the tiled area, and the table's sum of (A^2 + B^2 - 2 A B) is T^2
 *      times musica_sim_compare's sq_diff_sum of the region cut to (w / T) T x (h / T) T.
 *   2. DC: entry [0][0] holds the sum of (a tile's pixel sum)^2.
 *   3. Haar: 2 sum A^2 over sv, su >= T / 2 is T^2 sum (a[y][2 i] - a[y][2 i + 1])^2 over the tiled area, whatever T; and the sum A^2
 *      of column su = 1 is T times the sum, over the rows of every tile, of (left half's sum - right half's sum)^2.
 * A tile adds at most 2^40 to a word; a side is at most 16364, which gives at most 2^16 tiles at T = 64 and at most 2^22 tiles of at
 * most 2^28 at T = 8: every word stays below 2^63. Everything is an integer: the tables equal the restatement word for word and
 * repeat from call to call. Every word of the tables is written and nothing behind them. Synchronous, on the context's stream after
 * whatever was enqueued there; changes no slot, no result of a step and no input image; scratch is allocated on first use and regrown
 * when a call needs more. Refused before any device work: what musica_sim_compare refuses (with the smallest side 1 and at most
 * MUSICA_SPECTRUM_MAX_QUERIES queries, none included), then a tile that is not one of the four, a NULL `tables` and table_words below
 * the tables' words. After a refusal the context stays usable. */
#define MUSICA_SPECTRUM_WORDS 3
#define MUSICA_SPECTRUM_MAX_TILE 64
#define MUSICA_SPECTRUM_MAX_QUERIES 4
typedef struct musica_sim_spectrum_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t tiles;                 /* (w / T) * (h / T) */
} musica_sim_spectrum_result;
int musica_sim_spectrum(musica_ctx* ctx, uint32_t tile, uint32_t count, const musica_sim_query* queries,
                        musica_sim_spectrum_result* results, int64_t* tables, uint64_t table_words);

/* ---- texture: the gray-level co-occurrence matrices of a comparison (new, not in the reference) ----
 * Did the texture of the image survive? The second-order gray-level statistics of Haralick (1973), the terms in which radiomics
 * reports the stability of features under processing. metrics.cooccurrence_statistics is the contract. Queries are
 * musica_sim_compare's with w, h >= 1, at most MUSICA_COOCCURRENCE_MAX_QUERIES (a row's direct, registered and two vendor
 * comparisons). `levels` G is one of 8, 16, 32, 64: the level of an 8-bit pixel v is v >> (8 - log2 G). `distances` holds
 * distance_count = 1 .. MUSICA_COOCCURRENCE_MAX_DISTANCES distinct ascending d, each 1 .. MUSICA_COOCCURRENCE_MAX_DISTANCE. The four
 * directions of a distance d have the offsets (dx, dy), y running down: 0 degrees (d, 0), 45 (d, d), 90 (0, d), 135 (-d, d). Side a is
 * the graded plane of the query's image quantised as musica_sim_compare quantises it, side b the query's reference slot. A pair
 * (p, p + offset) counts on a side where BOTH pixels lie inside the region on that side, once, in T[level(p)][level(p + offset)]:
 * nothing is symmetrised. Query i gets distance_count * 4 * 2 * G * G uint32_t in the flat `tables`, from results[i].table_offset (in
 * words) on, indexed [distance][direction][side a = 0, b = 1][first level][second level]; results[i].pairs[k][direction] =
 * max(w - |dx|, 0) * max(h - dy, 0) for the distances given, 0 for the others. A region too small for an offset has no pair there and
 * an all-zero table: that is not a refusal. Identities: every [k][direction][side] table sums to pairs[k][direction]; its row and column
 * sums are the level histograms of the sub-rectangles that the first and the second pixels run over; the table at G / 2 is the 2 x 2
 * fold of the table at G. A side is at most 16364, so a table entry stays below 2^28 and uint32_t is exact. Everything is an integer:
 * the tables equal the restatement word for word and repeat from call to call, whatever MUSICA_COOCCURRENCE_GROUPS (the workgroups
 * of a query's distance and side, read at every call) says. Every word of the tables is written and nothing behind them. Synchronous,
 * on the context's stream after whatever was enqueued there; changes no slot, no result of a step and no input image; scratch is
 * allocated on first use. Refused before any device work: what musica_sim_compare refuses (with the smallest side 1 and at most
 * MUSICA_COOCCURRENCE_MAX_QUERIES queries, none included), then levels that are not one of the four, a NULL or empty or too long
 * distance list, a distance out of range or not above the one before it, a NULL `tables` and table_words below the tables' words.
 * After a refusal the context stays usable. */
#define MUSICA_COOCCURRENCE_MAX_DISTANCES 4
#define MUSICA_COOCCURRENCE_MAX_DISTANCE 16
#define MUSICA_COOCCURRENCE_MAX_LEVELS 64
#define MUSICA_COOCCURRENCE_MAX_QUERIES 4
typedef struct musica_sim_cooccurrence_result {
    uint64_t table_offset;          /* where the query's tables start in `tables`, in words */
    uint64_t pairs[MUSICA_COOCCURRENCE_MAX_DISTANCES][4];   /* [distance][direction]: the pairs that each of its two tables holds */
} musica_sim_cooccurrence_result;
int musica_sim_cooccurrence(musica_ctx* ctx, uint32_t levels, uint32_t distance_count, const uint32_t* distances, uint32_t count,
                            const musica_sim_query* queries, musica_sim_cooccurrence_result* results, uint32_t* tables, uint64_t table_words);

/* ---- size: the granulometry of a comparison (new, not in the reference) ----
 * Which object sizes became brighter or darker, and by how much? The granulometry of mathematical morphology (Matheron 1975; the
 * pattern spectrum of Maragos 1989): the openings and closings of an image by a growing element sieve its bright and its dark
 * structures by size, without inserting anything. metrics.granulometry_statistics is the contract. Queries are musica_sim_compare's
 * with w, h >= 1, at most MUSICA_GRANULOMETRY_MAX_QUERIES (a row's direct, registered and two vendor comparisons). Side a is the
 * graded plane of the query's image quantised as musica_sim_compare quantises it, side b the query's reference slot. The region is its
 * own domain: for r >= 1 the element of a pixel p is the (2 r + 1)^2 square around p CLIPPED to the region; the erosion is the minimum
 * over it, the dilation the maximum, the opening g_r the dilation of the erosion, the closing f_r the erosion of the dilation,
 * g_0 = f_0 = identity (scipy's minimum_filter with mode="constant", cval=255 and maximum_filter with cval=0 on the region's
 * sub-array). Nothing outside the region is read. So an interior bright square of side s survives g_r iff 2 r + 1 <= s, but a square
 * flush in the region's corner meets the clipped element and survives iff r + 1 <= s: a 3 x 3 square in the corner survives r = 2, one
 * in the interior is gone at r = 2. `radii` holds radius_count = 1 .. MUSICA_GRANULOMETRY_MAX_RADII distinct ascending
 * r_1 < .. < r_K, each 1 .. MUSICA_GRANULOMETRY_MAX_RADIUS, r_0 = 0. Query i gets (K + 1) * 2 * MUSICA_GRANULOMETRY_WORDS uint64_t in
 * the flat `tables`, from results[i].table_offset (in words) on, indexed [class][polarity bright = 0, dark = 1][word]. Class k < K:
 * bright A = g_{r_k}(a) - g_{r_k+1}(a), the bright structure that passes the sieve r_k and not r_k+1; dark
 * A = f_{r_k+1}(a) - f_{r_k}(a); class K, the residue: bright A = g_{r_K}(a), dark A = 255 - f_{r_K}(a); B likewise from b. Words:
 * sum A, sum B, sum A^2, sum B^2, sum A B over the region's pixels. Every A, B is 0 .. 255 and a side is at most 16364, so a word
 * stays below 2^45. results[i].pixels = w * h. Identities: the bright sums of A over the classes add up to sum a, the dark ones to
 * sum (255 - a) (B: b); complementing both sides swaps the polarities; swapping the sides swaps words 0 <-> 1 and 2 <-> 3; the table
 * is unchanged by the square's eight symmetries applied to both sides of the region; the sums of A and B of a coarser radii list are
 * the sums over the finer list's classes that a class spans. Everything is an integer: the tables equal the restatement word for word
 * and repeat from call to call, whatever MUSICA_GRANULOMETRY_GROUPS (the workgroups of a query's polarity, read at every call;
 * 0: the launch's own choice) says. Every word of the tables is written and nothing behind them. Synchronous, on the context's stream
 * after whatever was enqueued there; changes no slot, no result of a step and no input image; scratch is allocated on first use.
 * Refused before any device work: what musica_sim_compare refuses (with the smallest side 1 and at most
 * MUSICA_GRANULOMETRY_MAX_QUERIES queries, none included), then a NULL `radii`, a radius_count outside 1 ..
 * MUSICA_GRANULOMETRY_MAX_RADII, a radius out of range, a radius not above the one before it, a NULL `tables` and table_words below
 * the tables' words. After a refusal the context stays usable. */
#define MUSICA_GRANULOMETRY_MAX_RADII 8
#define MUSICA_GRANULOMETRY_MAX_RADIUS 16
#define MUSICA_GRANULOMETRY_MAX_QUERIES 4
#define MUSICA_GRANULOMETRY_WORDS 5
typedef struct musica_sim_granulometry_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t pixels;                /* w * h */
} musica_sim_granulometry_result;
int musica_sim_granulometry(musica_ctx* ctx, uint32_t radius_count, const uint32_t* radii, uint32_t count, const musica_sim_query* queries,
                            musica_sim_granulometry_result* results, uint64_t* tables, uint64_t table_words);

/* ---- contours: the distances between the edge sets of a comparison (new, not in the reference) ----
 * Are the contours of the output where the contours of the reference are, how far did they move, how many are new (halo rims, rebound
 * rings, noise lifted over the edge threshold) and how many are gone? musica_sim_gradients compares gradients at the same pixel; this
 * call compares the two edge SETS, as Pratt's figure of merit, the chamfer distances and the Hausdorff distance do, all of which come
 * from its table. metrics.contour_statistics is the contract. Queries are musica_sim_compare's with w, h >= 1, at most
 * MUSICA_CONTOURS_MAX_QUERIES (a row's direct, registered and two vendor comparisons). Side a is the graded plane of the query's image
 * quantised as musica_sim_compare quantises it, side b the query's reference slot. The region is its own domain; nothing outside it is
 * read. The contour E of a side: the strength M = gx^2 + gy^2 of the integer Sobel gradients (musica_sim_gradients') at
 * 1 <= x <= w - 2, 1 <= y <= h - 2 and 0 everywhere else (a region with a side below 3 has no contour); a pixel is horizontal where
 * |gx| >= |gy|, else vertical; before / after are M(x - 1, y) / M(x + 1, y) of a horizontal pixel, M(x, y - 1) / M(x, y + 1) of a
 * vertical one; E = M >= threshold and M > before and M >= after (on a plateau of equal strengths the left or upper pixel), threshold
 * 1 .. MUSICA_CONTOURS_MAX_THRESHOLD, the largest M there is. For a source set S and a target set T every pixel s of S gets
 * d2(s) = min over t in T of dx^2 + dy^2, exact; its bin is d2 where d2 <= radius^2 and radius^2 + 1 ("far") otherwise, radius
 * 1 .. MUSICA_CONTOURS_MAX_RADIUS; an empty T puts all of S into "far". Query i gets 2 * (radius^2 + 2) uint64_t in the flat `tables`,
 * from results[i].table_offset (in words) on, indexed [direction][bin]: direction 0 with S = E_a, T = E_b (where the output's contours
 * lie with respect to the reference's), direction 1 with S = E_b, T = E_a. A bin whose index is no sum of two squares is written as 0.
 * results[i].contour_a / contour_b = |E_a|, |E_b|, counted where the contours are made, not from the table; pixels = w * h. With
 * `planes` not NULL query i also gets w * h bytes, row-major, from results[i].plane_offset (in bytes; set whether or not planes were
 * asked for) on: bit 0 = E_a, bit 1 = E_b. Identities: row 0 sums to contour_a and row 1 to contour_b; table[0][0] == table[1][0] ==
 * |E_a and E_b|; swapping the sides swaps the rows; identical sides put everything into bin 0; the table at a smaller radius r is this
 * one with the bins r^2 + 1 .. radius^2 + 1 folded into its far bin; complementing either side (255 - v) changes nothing; the same
 * content at another origin gives the same table. Everything is an integer: tables and planes equal the restatement word for word
 * and repeat from call to call, whatever MUSICA_CONTOURS_GROUPS (the workgroups of a query's direction, read at every call; 0: the
 * launch's own choice) says. Every word of the tables is written and nothing behind them; with `planes` every byte of the planes and
 * nothing behind them. Synchronous, on the context's stream after whatever was enqueued there; changes no slot, no result of a step
 * and no input image; scratch is allocated on first use. Refused: what musica_sim_compare refuses (with the smallest side 1 and at
 * most MUSICA_CONTOURS_MAX_QUERIES queries, none included), then a threshold out of range, a radius out of range, a NULL `tables`,
 * table_words below the tables' words, and plane_bytes below the planes' bytes where `planes` is given; all before any launch or
 * copy. After a refusal the context stays usable. */
#define MUSICA_CONTOURS_MAX_RADIUS 32
#define MUSICA_CONTOURS_MAX_QUERIES 4
#define MUSICA_CONTOURS_MAX_THRESHOLD 1300500u
typedef struct musica_sim_contours_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t contour_a;             /* |E_a| */
    uint64_t contour_b;             /* |E_b| */
    uint64_t pixels;                /* w * h */
    uint64_t plane_offset;          /* where the query's byte plane starts in `planes`, in bytes */
} musica_sim_contours_result;
int musica_sim_contours(musica_ctx* ctx, uint32_t threshold, uint32_t radius, uint32_t count, const musica_sim_query* queries,
                        musica_sim_contours_result* results, uint64_t* tables, uint64_t table_words, uint8_t* planes, uint64_t plane_bytes);

/* ---- minkowski: the Minkowski functionals of the level sets of a comparison (new, not in the reference) ----
 * What does the gray-level landscape of the output look like as a shape: did the processing break one bright structure into islands,
 * punch holes into solid ones, lengthen the iso-contours? The answer is the three Minkowski functionals of every threshold set
 * {v >= t}: area, perimeter and Euler characteristic (components minus holes); by Hadwiger's theorem there is no fourth additive,
 * motion-invariant, continuous measure of a planar set. All of them, at all 255 thresholds, follow from the cell histograms that this
 * call returns. metrics.minkowski_statistics is the contract. Queries are musica_sim_compare's with w, h >= 1, at most
 * MUSICA_MINKOWSKI_MAX_QUERIES (a row's direct, registered and two vendor comparisons). The region is its own domain: pixels outside
 * it do not exist and nothing outside it is read. A side is a uint8 plane over the region: side 0 the graded plane of the query's image
 * quantised as musica_sim_compare quantises it, side 1 the query's reference slot, side 2 their pixel-wise minimum, whose upper sets
 * are the intersections of the two sides' upper sets. Query i gets MUSICA_MINKOWSKI_SIDES * MUSICA_MINKOWSKI_KINDS * 256 uint32_t
 * in the flat `tables`, from results[i].table_offset (in words) on, indexed [side][kind][v]: the number of cells of that kind whose
 * value is v. The kinds, their cells, their number and a cell's value:
 *   0 face     the pixels                                                   w h                the pixel
 *   1 any_h    the edges between horizontal neighbours, the two outline     h (w + 1)          the maximum of the 1 or 2 incident
 *              columns included                                                                pixels that exist
 *   2 any_v    the edges between vertical neighbours, the two outline       (h + 1) w          likewise
 *              rows included
 *   3 any_x    all pixel corners                                            (h + 1) (w + 1)    the maximum of the 1, 2 or 4 incident
 *                                                                                              pixels that exist
 *   4 all_h    the interior edges between horizontal neighbours             h (w - 1)          the minimum of the two
 *   5 all_v    the interior edges between vertical neighbours               (h - 1) w          the minimum of the two
 *   6 all_x    the interior corners                                         (h - 1) (w - 1)    the minimum of the four
 *   7 outline  the region's outline edges                                   2 w + 2 h          their one pixel (a corner pixel counts
 *                                                                                              twice, a 1 x 1 region's pixel four times)
 * Nothing is cumulated. On the closed cubical complex a cell belongs to the set at t iff the maximum of its incident pixels is >= t,
 * on the open complex iff their minimum is, so with N_k(t) the sum of row k over v >= t: area = N0; perimeter = N1 + N2 - N7 - N4 - N5,
 * the interior edges with exactly one side in the set (the crop is not charged); the Euler characteristic with 8-connected components
 * and 4-connected holes = N3 - N1 - N2 + N0, the one with 4-connected components and 8-connected holes = N0 - N4 - N5 + N6; the
 * outline edges that the set touches = N7 (metrics.minkowski_curves). results[i].pixels = w * h. Identities: every [side][kind] row
 * sums to the number of its cells above (a 1 x 1 region has three empty kinds); the sum over t >= 1 of the area is the sum of the
 * pixels, of the perimeter the sum of |differences| of horizontal and vertical neighbours; side 2's face row is the histogram of
 * min(a, b). Everything is an integer: the tables equal the restatement word for word and repeat from call to call, whatever
 * MUSICA_MINKOWSKI_GROUPS (the workgroups of a query's side, read at every call; 0: the launch's own choice) says. Every word of the
 * tables is written and nothing behind them. Synchronous, on the context's stream after whatever was enqueued there; changes no
 * slot, no result of a step and no input image; scratch is allocated on first use. Refused: what musica_sim_compare refuses (with
 * the smallest side 1 and at most MUSICA_MINKOWSKI_MAX_QUERIES queries, none included), then a NULL `tables` and table_words below
 * the tables' words; all before any launch or copy, `tables` untouched. After a refusal the context stays usable. */
#define MUSICA_MINKOWSKI_MAX_QUERIES 4
#define MUSICA_MINKOWSKI_KINDS 8
#define MUSICA_MINKOWSKI_SIDES 3
typedef struct musica_sim_minkowski_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t pixels;                /* w * h */
} musica_sim_minkowski_result;
int musica_sim_minkowski(musica_ctx* ctx, uint32_t count, const musica_sim_query* queries, musica_sim_minkowski_result* results,
                         uint32_t* tables, uint64_t table_words);

/* ---- reach: the change of the output by the distance from the changed input (new, not in the reference) ----
 * The locality relation: a change of the input inside a set changes the output only near that set. Two effects carry a local change
 * outwards: the pyramid's footprints (a level-i band reaches about 2^(i + 2) pixels and dies off with distance) and the global
 * stages (min / max, the two histograms, the tone curve: the same small shift everywhere, however far). Every other measurement scores
 * the place of the change, or the whole frame; this one keeps the exact sums of a comparison apart by the distance of the pixel from
 * the nearest CHANGED input pixel. metrics.reach_classes and metrics.reach_statistics are the contract; everything the device computes
 * is integer and bit-identical to them, from call to call as well.
 * The planes: "source" is the alteration source plane (musica_alter_set_source), "altered" the input plane that image `image_index`'s
 * current output was computed from (the plane the on-demand getters recompute from, also after a later alteration has overwritten
 * the input buffer), so input and output are always a coherent pair. seed = source != altered, over the whole N x N plane: seeds in
 * the MUSICA_OUT_MARGIN-pixel margin count, and distances are taken in the N x N plane.
 * The distance is Chebyshev's (L-infinity: the footprints of separable filters are squares). With K = radii_count radii, radii[0] = 0,
 * strictly ascending, each <= MUSICA_REACH_MAX_RADIUS, the class of input pixel (x, y) is the smallest k for which the box
 * [x - radii[k], x + radii[k]] x [y - radii[k], y + radii[k]], clipped to the plane, holds a seed, and K where the box of radii[K - 1]
 * holds none: class 0 is a changed pixel itself, class K "farther than the last radius, or nothing changed"; K + 1 classes.
 * A query is musica_sim_compare's (side a the 8-bit output of batch image `image_index`, quantised while read exactly as
 * musica_sim_compare reads it; side b reference slot `slot`; w, h >= 1). The class of a-side pixel (x, y) of the output plane is that
 * of input pixel (x + MUSICA_OUT_MARGIN, y + MUSICA_OUT_MARGIN), whatever origin side b has. Query i gets a table
 * [K + 1][MUSICA_REACH_WORDS] of uint64_t in the flat `tables`, from results[i].table_offset (in words: i * (K + 1) *
 * MUSICA_REACH_WORDS) on. A class's six words are the exact
 *   n, changed = the number of its pixels with a != b, sum_a, sum_b, sum_dd = sum of (a - b)^2, max_d = max |a - b| (0 for an empty class)
 * over the region's pixels of that class. INVARIANTS: the n of a table add up to w * h; results[i].ssd, the sum of its sum_dd, equals
 * musica_sim_compare's sq_diff_sum over the same region; changed <= n; max_d^2 * changed >= sum_dd >= changed. results[i].seeds is the
 * number of changed pixels of the N x N input plane, the same for every query of a call. Every word of the tables is written and
 * nothing behind them.
 * Both entry points are synchronous, on the context's stream after whatever was enqueued there; they change no slot, no input image
 * and no result of a step; scratch is grown on first use and freed with the context (the summed-area table of the seeds shares the
 * scatter calls' N x N u32 plane: no call needs both at once). Three launches: the seeds' prefix counts along the rows, running sums
 * down the columns, then the classes by bisection over the radii (four loads of the table a step) and the sums (kernels_reach.hip).
 * All queries of a call name the same image_index. Refused before any device work, musica_last_error naming the entry point: what
 * musica_sim_levels refuses about a context and its queries (sides from 1) with the largest count MUSICA_REACH_MAX_QUERIES; no source
 * plane; a last step whose input was not a plane of the context's (musica_execute_device); NULL radii; radii_count outside 1 ..
 * MUSICA_REACH_MAX_RADII; radii[0] != 0, radii that do not strictly ascend, a radius above MUSICA_REACH_MAX_RADIUS; queries that name
 * different images; a NULL `tables`; table_words < count * (K + 1) * MUSICA_REACH_WORDS. After a refusal the context stays usable. */
#define MUSICA_REACH_MAX_RADII 32
#define MUSICA_REACH_MAX_RADIUS 16383
#define MUSICA_REACH_MAX_QUERIES 16
#define MUSICA_REACH_WORDS 6
typedef struct musica_sim_reach_result {
    uint64_t table_offset;          /* where the query's table starts in `tables`, in words */
    uint64_t classes;               /* K + 1 */
    uint64_t ssd;                   /* sum over the region of (a - b)^2 */
    uint64_t pixels;                /* w * h */
    uint64_t seeds;                 /* changed pixels of the N x N input plane; the same for every query of a call */
} musica_sim_reach_result;
int musica_sim_reach(musica_ctx* ctx, uint32_t radii_count, const uint32_t* radii, uint32_t count, const musica_sim_query* queries,
                     musica_sim_reach_result* results, uint64_t* tables, uint64_t table_words);
/* The class plane itself: the (N - 20)^2 classes of the output plane's pixels as host bytes, row-major (metrics.reach_classes cropped
 * by MUSICA_OUT_MARGIN), for maps and for tests. The first two launches, then one that classifies and stores. Refused before any device
 * work: a NULL context or dst, an image too small for the margin, image_index >= batch, then what musica_sim_reach refuses about the
 * source, the last step's input and the radii. */
int musica_sim_reach_classes(musica_ctx* ctx, uint32_t image_index, uint32_t radii_count, const uint32_t* radii, uint8_t* dst);

/* ---- point response: defect pixels and clusters, the response stacked where they lie (new, not in the reference) ----
 * The impulse of the classical measurements: a single detector element or a small cluster is altered and the two-dimensional response
 * around it is read back, stacked over many positions. A multi-scale amplifier answers with a narrow core, a wide skirt and a rebound
 * ring of the opposite sign, differently for dead, faint and hot impulses and for different backgrounds. harness.insert_points,
 * harness.point_statistics and harness.point_summary are the contract; everything the device computes is integer and bit-identical to
 * them, from call to call as well (integer atomics and integer reductions: exact in any order).
 * A point is (x, y, radius, size, contrast, group): an integer pixel centre; MUSICA_POINT_MIN_RADIUS <= radius R <= MUSICA_POINT_MAX_RADIUS,
 * the half-side of its window; 1 <= size s <= MUSICA_POINT_MAX_SIZE; MUSICA_POINT_MIN_CONTRAST <= contrast <= MUSICA_POINT_MAX_CONTRAST
 * and not 0, in 1 / 1024 of the pixel's value; group < groups <= MUSICA_POINT_MAX_GROUPS. (The struct is musica_defect: musica_point is
 * the curves' (x, y).) Zones:
 *   window   |dx|, |dy| <= R            (side S = 2R + 1, at most 65: at most 4225 offsets). Every point of a list has the same R.
 *   cluster  along each axis the offsets -((s - 1) div 2) .. s div 2: s = 1 one pixel, s = 2 x .. x + 1, s = 3 x - 1 .. x + 1
 *   core     |dx|, |dy| <= 1            (holds every cluster)
 * A list for a plane of side n holds 1 .. MUSICA_POINT_MAX points whose windows lie inside [0, n)^2 and are pairwise disjoint
 * (|xi - xj| > 2R or |yi - yj| > 2R), so nothing depends on the list's order. Both entry points refuse every other list before any
 * device work.
 *   insertion   inside a cluster out = min((v * (1024 - contrast) + 512) >> 10, 65535), every other pixel copied. ONE rounding, halves
 *               up; contrast 1024 is a dead element (0), contrast -64512 multiplies by 64 and saturates everything above 1023 counts (a
 *               hot element); the largest intermediate is 65535 * 65536 + 512 < 2^32. UNLIKE the other patch relations an insertion
 *               with contrast > 512 CAN CREATE ZEROS (v = 1, contrast = 513 gives 0), which the noise and gradation histograms treat
 *               specially: that is what a dead element does to them, and part of what the rows measure.
 *   statistics  per point the sums of a and b over the 3 x 3 core and over the window, the window's sum of (a - b)^2 and its pixel
 *               count S^2; per group the stack, a uint32 table [3][S^2]: for every offset o = (dy + R) S + (dx + R), over all the
 *               group's points p, sum a(p + o), sum b(p + o) and sum (a - b)^2(p + o). Every window lies inside the plane, so every
 *               offset is hit by every point of the group: the count is the group's point count. A group without points is all zero.
 *               MUSICA_POINT_MAX * 255^2 = 266 342 400 < 2^32. `contrast` is not looked at, and `size` only checked.
 * For every group the stack's three sums over all offsets equal the sums of win_sum_a, win_sum_b and win_ssd over its points. As for the
 * details there is no musica_sim_..._reference sibling. */
#define MUSICA_POINT_MIN_RADIUS 4
#define MUSICA_POINT_MAX_RADIUS 32
#define MUSICA_POINT_MAX_SIZE 3
#define MUSICA_POINT_MIN_CONTRAST (-64512)
#define MUSICA_POINT_MAX_CONTRAST 1024
#define MUSICA_POINT_MAX_GROUPS 16
#define MUSICA_POINT_MAX 4096
typedef struct musica_defect {
    int32_t x, y;                   /* the centre, in pixels of the plane the call names */
    uint32_t radius;                /* MUSICA_POINT_MIN_RADIUS .. MUSICA_POINT_MAX_RADIUS, the same for every point of a list */
    uint32_t size;                  /* 1 .. MUSICA_POINT_MAX_SIZE */
    int32_t contrast;               /* MUSICA_POINT_MIN_CONTRAST .. MUSICA_POINT_MAX_CONTRAST, not 0, in 1 / 1024 of the pixel's value */
    uint32_t group;                 /* 0 .. groups - 1 */
} musica_defect;
typedef struct musica_sim_point_result {
    uint64_t core_sum_a, core_sum_b;   /* sums over the 3 x 3 core of side a (the output) and side b (the slot) */
    uint64_t win_sum_a, win_sum_b;     /* sums over the window */
    uint64_t win_ssd;                  /* sum over the window of (a - b)^2 */
    uint64_t win_pixels;               /* (2 radius + 1)^2 */
} musica_sim_point_result;
/* insert_points(source plane, points) into image `image_index` of the input buffer: the points are in the N x N plane's coordinates.
 * The kernel is enqueued on the ctx stream (the list is copied to the device first, which waits for what the stream holds), with
 * musica_alter's guarantees: it changes no other image of the input buffer, no result of the last step and no reference slot. One
 * launch, 2 bytes read and 2 written per pixel (kernels_points.hip). Refused before any device work: a NULL context or list, no source,
 * image_index >= batch, a count outside 1 .. MUSICA_POINT_MAX, a radius, size, contrast or group outside its limits, radii that differ,
 * a window that leaves the plane, two windows that are not disjoint. */
int musica_alter_points(musica_ctx* ctx, uint32_t image_index, uint32_t count, const musica_defect* points);
/* point_statistics of side a, the 8-bit output of batch image `image_index` (quantised while read, exactly as musica_sim_compare reads
 * it), against side b, reference slot `slot`: results[i] for points[i], in the coordinates of the (N - 20)^2 output plane, and the
 * groups' stacks, flat [groups][3][S^2], into `tables`, which holds table_words >= groups * 3 * S^2 words. Synchronous. win_ssd equals
 * musica_sim_compare's sq_diff_sum over the same S^2 region. Refused before any device work: a NULL context, list, results or tables, a
 * count outside 1 .. MUSICA_POINT_MAX, groups outside 1 .. MUSICA_POINT_MAX_GROUPS, an image too small for the margin, a slot out of
 * range or never written, image_index >= batch, a radius, size or group outside its limits, radii that differ, a window that leaves the plane,
 * two windows that are not disjoint, table_words too small. */
int musica_sim_points(musica_ctx* ctx, uint32_t image_index, uint32_t slot, uint32_t count, const musica_defect* points, uint32_t groups,
                      musica_sim_point_result* results, uint32_t* tables, uint64_t table_words);

/* ---- model observer: the channel responses of patches (new, not in the reference) ----
 * Task-based assessment puts a model observer on top of MTF, noise power and contrast-detail: it looks at a patch through a few
 * smooth channels and reports how well a signal is told from its absence against the background the processor produced (a
 * channelized Hotelling observer with Laguerre-Gauss channels: metrics.laguerre_gauss_bank, metrics.observer_summary). The device
 * does the expensive part, the inner products of many windows with a bank of templates; metrics.channel_responses is the contract,
 * and everything the device computes is integer and bit-identical to it, from call to call as well (no float, no atomics).
 * A bank is {half, channels, weights}: 1 <= half <= MUSICA_OBSERVER_MAX_HALF, the window |dx|, |dy| <= half of side S = 2 half + 1;
 * 1 <= channels C <= MUSICA_OBSERVER_MAX_CHANNELS; weights[C][S][S], row-major ([j][dy + half][dx + half]), the full int8 range. A
 * view is (x, y, bank): an integer centre in the (N - 20)^2 output plane and the index of its bank. A call holds 1 ..
 * MUSICA_OBSERVER_MAX_BANKS banks and 1 .. MUSICA_OBSERVER_MAX_VIEWS views whose windows lie inside the plane; they MAY overlap and
 * views may repeat (the call only reads). Side a is the 8-bit output of batch image `image_index`, quantised while read exactly as
 * musica_sim_compare reads it; side b is reference slot `slot`. View i gets 2 C int32_t in the flat `tables`, from
 * results[i].table_offset (in words; the tables lie one behind the other in view order) on: first the side-a responses
 *   R_a[j] = sum over dy, dx of weights[j][dy + half][dx + half] * a(x + dx, y + dy),   j = 0 .. C - 1,
 * then R_b[j] likewise; results[i].sum_a and sum_b are the window's plain sums. |R| <= 255 * 128 * 133^2 = 577 368 960 < 2^31 (asserted
 * below), so int32_t is exact. Every word of the tables is written and nothing behind them. Synchronous, on the context's stream
 * after whatever was enqueued there; changes no slot, no result of a step and no input image; scratch is allocated on first use.
 * One launch, one workgroup per view and block of 8 channels (kernels_observer.hip). Refused before any device work: a NULL context,
 * banks, views, results or tables; an image too small for the margin; a slot out of range or never written; image_index >= batch;
 * bank_count outside 1 .. MUSICA_OBSERVER_MAX_BANKS; a bank with NULL weights, or a half or channel count outside its limits; count
 * outside 1 .. MUSICA_OBSERVER_MAX_VIEWS; a view whose bank is not below bank_count or whose window leaves the plane; table_words
 * below the tables' total. After a refusal the context stays usable. */
#define MUSICA_OBSERVER_MAX_VIEWS 1024
#define MUSICA_OBSERVER_MAX_BANKS 8
#define MUSICA_OBSERVER_MAX_CHANNELS 16
#define MUSICA_OBSERVER_MAX_HALF 66          /* 2 * 32 + 2: the box of a radius-32 detail */
#ifdef __cplusplus
static_assert(255ll * 128 * (2 * MUSICA_OBSERVER_MAX_HALF + 1) * (2 * MUSICA_OBSERVER_MAX_HALF + 1) < (1ll << 31), "a channel response is an exact int32_t");
#endif
typedef struct musica_channel_bank {
    uint32_t half;                  /* 1 .. MUSICA_OBSERVER_MAX_HALF: the window |dx|, |dy| <= half, side S = 2 half + 1 */
    uint32_t channels;              /* 1 .. MUSICA_OBSERVER_MAX_CHANNELS */
    const int8_t* weights;          /* [channels][S][S], row-major, the full int8 range */
} musica_channel_bank;
typedef struct musica_view {
    int32_t x, y;                   /* the centre, in pixels of the output plane */
    uint32_t bank;                  /* 0 .. bank_count - 1 */
} musica_view;
typedef struct musica_sim_observer_result {
    uint64_t table_offset;          /* where the view's 2 x channels int32_t start in `tables`, in words */
    uint32_t pixels;                /* S^2 */
    uint32_t sum_a, sum_b;          /* the window's plain sums (<= 255 * 17689) */
} musica_sim_observer_result;
int musica_sim_observer(musica_ctx* ctx, uint32_t image_index, uint32_t slot, uint32_t bank_count, const musica_channel_bank* banks,
                        uint32_t count, const musica_view* views, musica_sim_observer_result* results, int32_t* tables, uint64_t table_words);

/* ---- device-resident output and stream ordering (new, not in the reference) ---- */

/* What musica_export_out writes per image. */
typedef enum musica_out_format {
    MUSICA_OUT_U8 = 0,          /* (N - 20) rows of N - 20 bytes: exactly musica_get_out_pixels' bytes (crop MUSICA_OUT_MARGIN, (uint8_t)(255 v)) */
    MUSICA_OUT_GRADED_F32 = 1,  /* N rows of N floats: exactly musica_get_graded's values */
    MUSICA_OUT_FORMAT_COUNT = 2
} musica_out_format;

/* Writes images first .. first + count - 1 of the last step into caller-owned DEVICE memory of the context's device: row r of image
 * first + k at d_dst + k * image_pitch_bytes + r * row_pitch_bytes; the bytes between rows and between images are left alone.
 * Enqueued on the context's stream behind whatever is there (a step, musica_execute_device, a pipeline step of this context, the last
 * batch of musica_execute_stream); returns without waiting. Changes no result of the step and no other buffer. Refused before
 * anything is enqueued when ctx or d_dst is NULL, the format is out of range, count is 0 or first + count exceeds the batch, a pitch
 * is smaller than a row (row_pitch < width bytes) or an image (image_pitch < row_pitch * rows), with MUSICA_OUT_GRADED_F32 when
 * d_dst or a pitch is not a multiple of 4, with MUSICA_OUT_U8 when N <= 20, when no step has run on the context, when d_dst is not
 * device memory of the context's device (pinned and pageable host memory are refused) and when the last byte written lies beyond
 * the allocation that holds d_dst. */
int musica_export_out(musica_ctx* ctx, uint32_t first, uint32_t count, uint32_t format, void* d_dst, size_t row_pitch_bytes,
                      size_t image_pitch_bytes);

/* Stream ordering with a caller's stream (a hipStream_t of the context's device; NULL = the null stream). musica_stream_wait: all
 * that the context enqueues from now on (steps, exports, stats, similarity, alterations) starts after the work already on `stream`.
 * musica_stream_signal: the work enqueued on `stream` from now on starts after everything enqueued on the context so far (the side
 * stream of a two-stream context rejoins the context's stream inside every step, eager or replayed). Neither waits on the host.
 * Refused for a stream of another device and for a stream that is capturing a graph. */
int musica_stream_wait(musica_ctx* ctx, void* stream);
int musica_stream_signal(musica_ctx* ctx, void* stream);

/* ---- test / profiling hooks ------------------------------------------ */

/* A sequence of `count` batches (pixels[j]: batch x N x N uint16 in host memory), pipelined: two device input buffers and a
 * copy stream, so the host-to-device copy of batch j + 1 runs under the kernels of batch j — what replaces the reference's
 * staging-buffer upload with three queue-idle waits per image (VulkanState::loadDataToImage, src/vk_state.cpp:313-342).
 * Returns after the last batch has been computed; the context then holds the results of batch count - 1 (every getter works).
 * stats (may be NULL): count * batch rows, row j * batch + i = image i of batch j, image_id = its index in the sequence.
 * Inputs in pinned memory (musica_host_alloc) are copied at the PCIe rate; pageable memory is accepted (slower). */
int musica_execute_stream(musica_ctx* ctx, const uint16_t* const* pixels, uint32_t count, musica_stats* stats);
/* Page-locked host memory for musica_execute_stream / musica_execute inputs (hipHostMalloc / hipHostFree). */
void* musica_host_alloc(musica_ctx* ctx, size_t bytes);
void musica_host_free(musica_ctx* ctx, void* ptr);

/* Overwrites one stored intermediate of one batch entry (dense f32 in). Only
 * kinds the hot path keeps resident are accepted. */
int musica_debug_set_image(musica_ctx* ctx, uint32_t image_index, musica_image_kind kind, uint32_t level, const float* src);
/* Runs exactly one stage of the dispatch script on the current device state. */
int musica_debug_run_stage(musica_ctx* ctx, musica_stage stage);

/* Per-kernel device timing with HIP events on the ctx stream.
 * musica_profile_enable(ctx, mask): mask < 0 brackets every kernel family of every
 * later execute with an event pair, mask > 0 only the families whose bit
 * (1 << musica_kernel_id) is set, 0 switches it off. musica_profile_get returns
 * the mean duration in microseconds and the launch count since the last reset. */
typedef enum musica_kernel_id {
    MUSICA_KERNEL_MINMAX = 0,
    MUSICA_KERNEL_NORMALIZE = 1,
    MUSICA_KERNEL_REDUCE_L0 = 2,   /* fused 5-tap smooth + 2x downsample at level 0 (the metric kernel) */
    MUSICA_KERNEL_REDUCE_REST = 3, /* same kernel, levels >= 1 */
    MUSICA_KERNEL_BAND_L0 = 4,     /* fused upsample + smooth x4 + difference at level 0 */
    MUSICA_KERNEL_BAND_REST = 5,
    MUSICA_KERNEL_SDEV_HIST = 6,
    MUSICA_KERNEL_CURVES = 7,
    MUSICA_KERNEL_CNR = 8,
    MUSICA_KERNEL_EXPAND_L0 = 9,   /* fused contrast apply + NR + upsample + smooth x4 + addition at level 0 */
    MUSICA_KERNEL_EXPAND_REST = 10,
    MUSICA_KERNEL_GRAD_HIST = 11,
    MUSICA_KERNEL_GRAD_CURVE = 12,
    MUSICA_KERNEL_GRAD_APPLY = 13,
    MUSICA_KERNEL_COUNT = 14
} musica_kernel_id;
int musica_profile_enable(musica_ctx* ctx, int mask);
int musica_profile_reset(musica_ctx* ctx);
int musica_profile_get(musica_ctx* ctx, musica_kernel_id id, double* mean_us, uint64_t* launches);

/* Stand-alone launch of the metric kernel (fused smooth + downsample) on a
 * side x side f32 image owned by the caller in device memory (pitch in floats,
 * multiple of 4). Used by bench.py to time the kernel at 4096 x 4096 and by the
 * kernel-level parity tests. d_out has side ceil(side/2), pitch out_pitch. */
int musica_k_reduce(musica_ctx* ctx, const float* d_in, uint32_t side, uint32_t in_pitch,
                    float* d_out, uint32_t out_pitch, uint32_t batch);
/* Times `iters` back-to-back launches of the above with HIP events on the ctx
 * stream; returns mean microseconds per launch in *mean_us. */
int musica_k_reduce_timed(musica_ctx* ctx, const float* d_in, uint32_t side, uint32_t in_pitch,
                          float* d_out, uint32_t out_pitch, uint32_t batch, uint32_t iters, double* mean_us);

/* The same measurement from HBM rather than from the 256 MiB Infinity Cache: launch i uses input plane
 * d_in + (i % nbuf) * in_pitch * side and output plane d_out + (i % nbuf) * out_pitch * ceil(side/2), so with
 * nbuf * 5 * side^2 bytes well above 256 MiB no launch finds its input (or the lines of its output) on the die. */
int musica_k_reduce_timed_rot(musica_ctx* ctx, const float* d_in, uint32_t side, uint32_t in_pitch, float* d_out,
                              uint32_t out_pitch, uint32_t nbuf, uint32_t iters, double* mean_us);
/* Measurement aid, not on the product path: a plain streaming kernel with the metric kernel's traffic shape
 * (reads side^2 f32 with 16-byte loads, writes (side/2)^2 f32 with 16-byte stores, no halo, no arithmetic to
 * speak of), timed the same rotating way — the ceiling `roofline.frac` can be read against. side % 8 == 0,
 * dense rows. */
int musica_k_copy41_timed_rot(musica_ctx* ctx, const float* d_in, uint32_t side, float* d_out, uint32_t nbuf,
                              uint32_t iters, double* mean_us);

/* Self-test of the exact arithmetic shortcuts that lean on a hardware approximation (v_rsq_f32) and therefore
 * cannot be checked on a CPU (csrc/exact_math.h): runs on the ctx device over EVERY float bit pattern and counts
 * disagreements with the literal expressions of the shaders (img_sqrt.comp:15, img_sdev.comp:30,
 * img_normalize.comp:24). mismatches[0]: musica_sqrt vs sqrtf, 2^32 patterns; [1]: the 8-wide grouped form;
 * [2]: the grouped form with a +0 among the eight; [3]: the normalisation of a raw pixel for every
 * (pixel, min, max) triple the chains can produce (65536 x 256 x 256). All four must be 0. */
int musica_selftest_exact_math(musica_ctx* ctx, uint64_t mismatches[4]);

/* Raw device memory helpers so callers without a HIP binding (ctypes tests,
 * bench.py) can stage buffers for the two functions above. */
void* musica_device_alloc(musica_ctx* ctx, size_t bytes);
void musica_device_free(musica_ctx* ctx, void* d_ptr);
int musica_memcpy_h2d(musica_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int musica_memcpy_d2h(musica_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ---- file formats (host only, no GPU needed) -------------------------- */

/* Raw reader of test/standalone/main.cpp:54-75: file = 256-byte header
 * (ignored) + N*N little-endian uint16, size must match exactly. */
int musica_read_raw(const char* path, uint32_t image_size, uint16_t* dst);
/* 24-bpp BMP writer byte-identical to stbi_write_bmp(path, w, h, 1, data). */
int musica_write_bmp_gray(const char* path, uint32_t w, uint32_t h, const uint8_t* data);
/* 32-bpp BMP writer byte-identical to stbi_write_bmp(path, w, h, 4, data) (V4 header, stb_image_write.h:501-509). */
int musica_write_bmp_rgba(const char* path, uint32_t w, uint32_t h, const uint8_t* data);

/* ---- misc ------------------------------------------------------------ */
const char* musica_last_error(void);
uint32_t musica_abi_version(void);
/* Number of HIP devices visible; 0 when there is none (never falls back to a CPU path). */
int musica_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* MUSICA_H */
