// musica_ctx.h — the context behind include/musica.h's opaque musica_ctx and what its host files share: musica_ctx.hip (create, queries,
// getters, dumps), musica_step.hip (the form of a step and its launch sequence, graphs, autotune, lanes, the execute entry points),
// musica_pipeline.hip (musica_pipeline_*) and musica_study.hip (musica_sim_* / musica_alter_*). Internal: not installed.
#pragma once

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <exception>
#include <vector>

#include "launchers.h"

using namespace musica;

#define HIDDEN __attribute__((visibility("hidden")))
// Records the message for musica_last_error, prints it and returns 0 (musica_ctx.hip).
HIDDEN int fail(const char* fmt, ...);
static inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// No C++ exception may cross the extern "C" boundary (a ctypes / CLI caller would abort): entry points that allocate
// host memory run their body under this guard and report through fail() like every other error.
#define ABI_TRY try {
#define ABI_CATCH(name_)                                                                             \
    }                                                                                                \
    catch (const std::exception& e_) { return fail("%s: %s", name_, e_.what()); }                   \
    catch (...) { return fail("%s: unknown C++ exception", name_); }

#define HIP_OK(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s", #call, hipGetErrorString(e_));  \
    } while (0)

// ---- context --------------------------------------------------------------------------
struct ProfSpan {
    int id;
    hipEvent_t a, b;
};

// Captured graphs kept per context, one per distinct input pointer (include/musica.h, musica_execute_device).
constexpr int kGraphSlots = 4;
constexpr int kLaneStreams = 1;   // streams of the image lanes (musica_ctx::lanes). One: a one-image chain (0.14 - 0.19 ms) is as long as an image's copy,
                                  // so chains on several streams would barely overlap, and which hardware queue a further stream lands on (4 queues,
                                  // round-robin over every stream of the process) decided whether three lanes were faster or slower than none

// Every device buffer that holds one slice per image: B slices, image k's at k x its elements per image. for_each_buffer names each
// member once with that count; allocation, the image lanes and the getters all go through it.
struct DeviceBuffers {
    uint16_t* d_input = nullptr;
    uint32_t* d_minmax = nullptr;
    uint32_t* d_mm_slots = nullptr;    // [B][kMinMaxSlots]: per-block {min | max << 16} of k_minmax_u16
    uint32_t* d_mm_ticket = nullptr;   // [B]: its arrival counters (self-resetting)
    uint32_t* d_gr_ticket = nullptr;   // [B][kGradTicketStride]: the tickets of the one-launch recount + tone curve
    float* d_norm = nullptr;
    float* d_down[MUSICA_MAX_LEVELS] = {};
    float* d_band[MUSICA_MAX_LEVELS] = {};
    float* d_recon[MUSICA_MAX_LEVELS] = {};
    float* d_sdev[4] = {};
    uint32_t* d_noise_hist = nullptr;
    musica_hist_max_point* d_noise_max = nullptr;
    DevCurve* d_curves = nullptr;
    DevCurveLut* d_luts = nullptr;
    float* d_cnr = nullptr;
    uint32_t* d_grad_hist = nullptr;
    uint32_t* d_grad_hist_b = nullptr;   // the literal recount of images whose reconstruction holds an exact zero (fused gradation histogram)
    uint32_t* d_gzero = nullptr;         // [B]: that condition
    int* d_thr090 = nullptr;             // [B]: raw-pixel form of `normalized <= 0.9`
    double* d_stats_partial = nullptr;   // [B][kStatsMaxBlocks]: partial sums of the cnr image (k_stats_partial -> k_stats)
    uint16_t* d_le090 = nullptr;         // [B][S1][S0 / 8] or null: its bit image, written by the level-0 reduce + band launch for the level-0 expand launch
    musica_hist_max_point* d_grad_max = nullptr;
    DevCurve* d_gcurve = nullptr;
    float* d_graded = nullptr;
    float* d_scratch = nullptr;
    musica_stats* d_stats = nullptr;
    uint32_t* d_clahe_hist = nullptr;
    musica_point* d_clahe_pts = nullptr;
    float* d_clahe_graded = nullptr;
};

// What the study's entry points keep between calls (musica_study.hip): context-level, every buffer allocated on first use.
struct StudyState {
    // musica_sim_*: the reference slots (u8, side N - 20) and which of them hold a plane
    uint8_t* slot[MUSICA_SIM_SLOTS] = {};
    bool written[MUSICA_SIM_SLOTS] = {};
    uint16_t* d_vendor = nullptr;    // musica_sim_set_vendor_reference's staging plane: (N - 20)^2 u16 (u8 data uses its first half)
    // musica_sim_compare
    SimQueryDev* d_sim_q = nullptr;
    SimPart* d_sim_part = nullptr;   // [MUSICA_SIM_MAX_QUERIES][kSimMaxBlocks]
    SimPart* d_sim_out = nullptr;    // [MUSICA_SIM_MAX_QUERIES]
    uint32_t* d_sim_hist = nullptr;  // [MUSICA_SIM_MAX_QUERIES][512]: value counts of a, then b
    // musica_sim_joint
    JointQueryDev* d_joint_q = nullptr;
    uint32_t* d_joint = nullptr;     // [MUSICA_SIM_MAX_QUERIES][65536]: J[a][b], row a
    // musica_sim_displace
    DisplaceQueryDev* d_disp_q = nullptr;
    unsigned long long* d_disp_tables = nullptr;   // [MUSICA_SIM_MAX_QUERIES][33 * 33]
    uint32_t* d_disp_off = nullptr;                // [MUSICA_SIM_MAX_QUERIES]: tiles_off
    uint32_t* d_disp_tiles = nullptr;              // the tile tables of one call: disp_tiles_cap u32, regrown when a call needs more
    size_t disp_tiles_cap = 0;
    // musica_sim_multiscale
    ScalePoolDev* d_scale_q = nullptr;             // [MUSICA_SIM_MAX_QUERIES]
    ScaleJobDev* d_scale_jobs = nullptr;           // [MUSICA_SIM_MAX_QUERIES * MUSICA_SIM_MAX_SCALES]
    ScaleWinPart* d_scale_part = nullptr;          // [jobs][kScaleMaxBlocks]
    ScaleOut* d_scale_out = nullptr;               // [jobs]
    uint8_t* d_scale_planes = nullptr;             // the pooled planes of one call: scale_planes_cap bytes, regrown when a call needs more
    size_t scale_planes_cap = 0;
    ScalePoolPart* d_scale_pool = nullptr;         // the tiles' partials of one call: scale_pool_cap elements, likewise
    size_t scale_pool_cap = 0;
    // musica_sim_ensemble_*
    uint2* d_ens = nullptr;                        // [(N - 20)^2]: {S1, S2} per output pixel, allocated by the first reset
    uint32_t ens_k = 0;                            // realisations added since the last reset
    bool ens_reset = false;                        // a reset has been enqueued: the accumulators exist and start from zero
    EnsQueryDev* d_ens_q = nullptr;                // [MUSICA_SIM_MAX_QUERIES]
    unsigned long long* d_ens_out = nullptr;       // [MUSICA_SIM_MAX_QUERIES][kEnsTotals]
    unsigned long long* d_ens_tiles = nullptr;     // the tile pairs of one call: 2 * ens_tiles_cap u64, regrown when a call needs more
    size_t ens_tiles_cap = 0;
    // musica_sim_ensemble_track / _covariance: the tracked regions of the ensemble now running (none after a reset)
    uint32_t cov_regions = 0, cov_radius = 0;      // cov_regions == 0: nothing is tracked and musica_sim_ensemble_add launches k_ens_add alone
    int cov_max_tiles = 1;
    size_t cov_words = 0;                          // u64 per tile-table buffer of the regions tracked now
    musica_sim_query cov_q[MUSICA_SIM_COV_MAX_REGIONS] = {};
    CovRegionDev* d_cov_r = nullptr;               // [MUSICA_SIM_COV_MAX_REGIONS]
    unsigned long long* d_cov_tiles = nullptr;     // the tiles' P(d): cov_tiles_cap u64, regrown when a track call needs more
    long long* d_cov_ctiles = nullptr;             // the tiles' C(d) of the last covariance call, the same size
    size_t cov_tiles_cap = 0;
    unsigned long long* d_cov_tables = nullptr;    // [MUSICA_SIM_COV_MAX_REGIONS][17 * 33]
    // musica_alter_*: the source plane (N x N u16), the radix-select counts and the fill
    uint16_t* d_alter_src = nullptr;
    uint32_t* d_alter_hist = nullptr;    // [768]
    double* d_alter_fill = nullptr;      // [1]
    int32_t* d_alter_draws = nullptr;    // [N * N], musica_alter_draws only
    // musica_alter_scatter / musica_sim_scatter_reference: the row passes' plane between the two launches
    uint32_t* d_scatter = nullptr;       // [N * N] (a slot's (N - 20)^2 use its start), allocated by the first scatter call
    // musica_alter_warp / musica_sim_warp_reference: the device copy of the call's nodes, one u32 each
    uint32_t* d_warp_nodes = nullptr;    // warp_nodes_cap nodes, regrown when a call needs more
    size_t warp_nodes_cap = 0;
    // musica_alter_details / musica_sim_details: the device copy of the call's detail list and the details' sums
    PackedDetail* d_details = nullptr;             // [MUSICA_DETAIL_MAX], allocated by the first call of either
    unsigned long long* d_detail_out = nullptr;    // [MUSICA_DETAIL_MAX][kDetailWords], allocated by the first musica_sim_details
    // musica_alter_edges / musica_sim_edges: the device copy of the call's edge list, the edges' results and their flat tables
    PackedEdge* d_edges = nullptr;                 // [MUSICA_EDGE_MAX], allocated by the first call of either
    unsigned long long* d_edge_out = nullptr;      // [MUSICA_EDGE_MAX][kEdgeWords], allocated by the first musica_sim_edges
    uint32_t* d_edge_tables = nullptr;             // [MUSICA_EDGE_MAX][4][MUSICA_EDGE_BINS_MAX] (8 MiB), allocated by the first musica_sim_edges
    // musica_alter_gratings / musica_sim_gratings: the device copy of the call's grating list, its waves, the results and the flat tables
    PackedGrating* d_gratings = nullptr;           // [MUSICA_GRATING_MAX], allocated by the first call of either
    int16_t* d_grating_waves = nullptr;            // [MUSICA_GRATING_MAX][MUSICA_GRATING_MAX_PERIOD], allocated by the first musica_alter_gratings
    unsigned long long* d_grating_out = nullptr;   // [MUSICA_GRATING_MAX][kGratingWords], allocated by the first musica_sim_gratings
    uint32_t* d_grating_tables = nullptr;          // [MUSICA_GRATING_MAX][4][MUSICA_GRATING_MAX_PERIOD] (256 KiB), allocated by the first musica_sim_gratings
    // musica_alter_gain: the device copy of the call's tables; musica_sim_profiles: the queries and the flat tables
    uint16_t* d_gain_x = nullptr;                  // [N], allocated by the first musica_alter_gain
    uint32_t* d_gain_y = nullptr;                  // [N]: gy widened to u32, likewise
    ProfileQueryDev* d_profile_q = nullptr;        // [MUSICA_PROFILE_MAX_QUERIES]
    uint32_t* d_profile_tables = nullptr;          // the tables of one call: profile_tables_cap u32, regrown when a call needs more
    size_t profile_tables_cap = 0;
    // musica_alter_lut: the device copy of the call's table; musica_sim_levels: the queries and the flat tables
    uint16_t* d_lut = nullptr;                     // [kLutEntries] (128 KiB), allocated by the first musica_alter_lut
    LevelQueryDev* d_level_q = nullptr;            // [MUSICA_LEVEL_MAX_QUERIES]
    unsigned long long* d_level_tables = nullptr;  // [MUSICA_LEVEL_MAX_QUERIES][kLevelMaxClasses][kLevelWords] (768 KiB), allocated by the first musica_sim_levels
    // musica_sim_gradients: the queries, the flat tables, the sums of q and the tiles' partials
    GradQueryDev* d_grad_q = nullptr;              // [MUSICA_SIM_MAX_QUERIES]
    unsigned long long* d_grad_tables = nullptr;   // [MUSICA_SIM_MAX_QUERIES][kGradClasses][kGradWords], allocated by the first musica_sim_gradients
    double* d_grad_out = nullptr;                  // [MUSICA_SIM_MAX_QUERIES]
    double* d_grad_part = nullptr;                 // the tiles' partials of one call: grad_part_cap doubles, regrown when a call needs more
    size_t grad_part_cap = 0;
    // musica_sim_order: the queries and the flat tables
    OrderQueryDev* d_order_q = nullptr;            // [MUSICA_SIM_MAX_QUERIES]
    unsigned long long* d_order_tables = nullptr;  // [MUSICA_SIM_MAX_QUERIES][kOrderTableWords], allocated by the first musica_sim_order
    // musica_sim_lattice: the queries and the flat tables
    LatticeQueryDev* d_lattice_q = nullptr;          // [MUSICA_LATTICE_MAX_QUERIES]
    unsigned long long* d_lattice_tables = nullptr;  // [MUSICA_LATTICE_MAX_QUERIES][kLatticeMaxPeriod^2][kLatticeWords], allocated by the first musica_sim_lattice
    uint32_t* d_lattice_part = nullptr;              // the workgroups' partial tables of one call: lattice_part_cap words, regrown when a call needs more
    size_t lattice_part_cap = 0;
    // musica_sim_blobs: the queries, the flat tables and the scratch of one call (kernels_blobs.hip: BlobScratch), each regrown when a
    // call needs more
    BlobQueryDev* d_blob_q = nullptr;               // [MUSICA_BLOBS_MAX_QUERIES]
    unsigned long long* d_blob_tables = nullptr;    // [MUSICA_BLOBS_MAX_QUERIES][kBlobClasses][kBlobWords], allocated by the first musica_sim_blobs
    uint32_t* d_blob_parent = nullptr;              // blob_plane_cap words, and as many in d_blob_slots
    uint32_t* d_blob_slots = nullptr;
    size_t blob_plane_cap = 0;
    uint32_t* d_blob_labels = nullptr;              // blob_label_cap words: only calls that ask for label planes
    size_t blob_label_cap = 0;
    BlobRecord* d_blob_recs = nullptr;              // blob_tile_cap tiles of kBlobTileRecords records, and as many words in d_blob_counts
    uint32_t* d_blob_counts = nullptr;
    size_t blob_tile_cap = 0, blob_count_cap = 0;
    unsigned long long* d_blob_best = nullptr;      // [kBlobMaxQueries] keys, then one word of errors (as u64)
    BlobBest* d_blob_largest = nullptr;             // [kBlobMaxQueries]
    // musica_sim_spectrum: the queries and the flat tables
    SpectrumQueryDev* d_spectrum_q = nullptr;         // [MUSICA_SPECTRUM_MAX_QUERIES]
    unsigned long long* d_spectrum_tables = nullptr;  // [MUSICA_SPECTRUM_MAX_QUERIES][kSpectrumMaxTile^2][kSpectrumWords], allocated by the first musica_sim_spectrum
    unsigned long long* d_spectrum_part = nullptr;    // the workgroups' partial tables of one call: spectrum_part_cap words, regrown when a call needs more
    size_t spectrum_part_cap = 0;
    // musica_sim_cooccurrence: the queries and the flat tables
    CooccurrenceQueryDev* d_cooccurrence_q = nullptr;   // [MUSICA_COOCCURRENCE_MAX_QUERIES]
    uint32_t* d_cooccurrence_tables = nullptr;          // [MUSICA_COOCCURRENCE_MAX_QUERIES][MAX_DISTANCES][4][2][MAX_LEVELS^2], allocated by the first musica_sim_cooccurrence
    // musica_sim_granulometry: the queries and the flat tables
    GranulometryQueryDev* d_granulometry_q = nullptr;         // [MUSICA_GRANULOMETRY_MAX_QUERIES]
    unsigned long long* d_granulometry_tables = nullptr;      // [MUSICA_GRANULOMETRY_MAX_QUERIES][MAX_RADII + 1][2][MUSICA_GRANULOMETRY_WORDS], allocated by the first musica_sim_granulometry
    // musica_sim_contours: the queries, the flat tables, the set sizes and the scratch planes
    ContourQueryDev* d_contour_q = nullptr;                   // [MUSICA_CONTOURS_MAX_QUERIES]
    unsigned long long* d_contour_tables = nullptr;           // [MUSICA_CONTOURS_MAX_QUERIES][2][MAX_RADIUS^2 + 2], allocated by the first musica_sim_contours
    unsigned long long* d_contour_counts = nullptr;           // [MUSICA_CONTOURS_MAX_QUERIES][2]: |E_a|, |E_b|
    unsigned long long* d_contour_bits = nullptr;             // contour_bits_cap words: per query the two sides' bit planes, h rows of ceil(w / 64) words
    size_t contour_bits_cap = 0;
    uint8_t* d_contour_planes = nullptr;                      // contour_plane_cap bytes: only calls that ask for the byte planes
    size_t contour_plane_cap = 0;
    // musica_sim_minkowski: the queries and the flat tables
    MinkowskiQueryDev* d_minkowski_q = nullptr;               // [MUSICA_MINKOWSKI_MAX_QUERIES]
    uint32_t* d_minkowski_tables = nullptr;                   // [MUSICA_MINKOWSKI_MAX_QUERIES][SIDES][KINDS][256], allocated by the first musica_sim_minkowski
    // musica_sim_reach / musica_sim_reach_classes: the radii, the queries, the flat tables and the class plane. The summed-area table
    // of the change mask lives in d_scatter: every call that uses that plane fills it itself and is done with it when it returns.
    uint32_t* d_reach_radii = nullptr;             // [MUSICA_REACH_MAX_RADII], allocated by the first call of either
    ReachQueryDev* d_reach_q = nullptr;            // [MUSICA_REACH_MAX_QUERIES]
    unsigned long long* d_reach_tables = nullptr;  // [MUSICA_REACH_MAX_QUERIES][MUSICA_REACH_MAX_RADII + 1][kReachWords]
    uint8_t* d_reach_classes = nullptr;            // [(N - 20)^2], allocated by the first musica_sim_reach_classes
    // musica_alter_points / musica_sim_points: the device copy of the call's point list, the points' results, the stacks and the launch plan
    PackedPoint* d_points = nullptr;               // [MUSICA_POINT_MAX + kPointTileRows] (point_rows' entries behind an insertion's list), allocated by the first call of either
    unsigned long long* d_point_out = nullptr;     // [MUSICA_POINT_MAX][kPointWords], allocated by the first musica_sim_points
    uint32_t* d_point_tables = nullptr;            // [kPointTableWords] stacks (792 KiB), then [kPointPlanWords] of point_plan, allocated likewise
    // musica_sim_observer: the device copy of the call's views, its banks' packed weights, the flat tables and the windows' plain sums
    PackedView* d_obs_views = nullptr;             // [MUSICA_OBSERVER_MAX_VIEWS], allocated by the first call
    uint32_t* d_obs_weights = nullptr;             // observer_pack's words of one call: obs_weights_cap u32, regrown when a call needs more
    size_t obs_weights_cap = 0;
    int32_t* d_obs_tables = nullptr;               // [MUSICA_OBSERVER_MAX_VIEWS][2][MUSICA_OBSERVER_MAX_CHANNELS] (128 KiB), allocated by the first call
    uint32_t* d_obs_sums = nullptr;                // [MUSICA_OBSERVER_MAX_VIEWS][2], likewise
};

struct musica_ctx : DeviceBuffers {
    musica_params p;
    musica_tunables tun;     // the constants of the host parameter formulas (musica_create_ex; default: the reference's)
    int N, L, B;
    bool generic;
    int ref_order;           // MUSICA_FLAG_REFERENCE_ORDER: generic kernels in the shaders' literal 25-tap accumulation order
    LevelDesc lv[MUSICA_MAX_LEVELS + 1];
    int min_chain_exact;
    int hist_cov;  // (N / 512) * 512
    hipStream_t stream = nullptr;
    hipStream_t cur;         // stream the run_*_level helpers launch on (stream or side)
    hipStream_t side = nullptr;   // coarse-level chain runs here, concurrently with the level-0 kernels on `stream`
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool fuse_u16;           // level-0 kernels read the raw uint16 pixels; the normalized image is produced on demand only
    bool grad_one_launch;    // recount + tone curve in one launch behind the fused expand launch (MUSICA_GRAD_ONE_LAUNCH=0: two)
    bool tiny_tail;          // levels of side <= kTailSide in one launch (MUSICA_TINY_TAIL=0: one launch per level and stage)
    bool clahe_one_apply;    // ... and whose two apply passes are one launch (MUSICA_CLAHE_ONE_APPLY=0: k_grad_apply and k_clahe_apply4)
    bool clahe_in_expand;    // ... and whose histogram the level-0 expand launch counts (MUSICA_CLAHE_IN_EXPAND=0: k_clahe_hist)
    bool clahe_raw;          // CLAHE context whose relevant image is computed from the raw pixels (no stored normalized image)
    bool norm_valid = false; // d_norm holds the normalized image of the current input
    // hipGraph replay of the two-stream dispatch (captured once per input pointer; MUSICA_FLAG_NO_GRAPH /
    // MUSICA_GRAPH=0 / per-kernel profiling fall back to eager launches)
    bool use_graph;
    hipGraphExec_t graph_exec[kGraphSlots] = {};      // one captured graph per input pointer, the kGraphSlots most recently used (the streaming
    const uint16_t* graph_input[kGraphSlots] = {};    // path alternates between two device input buffers; callers may rotate a few of their own)
    uint64_t graph_used[kGraphSlots] = {};            // launch counter at the slot's last use (least recently used slot is recaptured)
    uint64_t graph_clock = 0;
    int dag;                 // 0: one in-order stream (enqueue_one_stream); 2: two streams (enqueue_two_streams: the analysis beside the reduce tail)
    // device state shared by the whole context (the per-image buffers are the DeviceBuffers base)
    uint16_t* d_input2 = nullptr;      // second input buffer of the streaming path (musica_execute_stream), allocated on first use
    hipStream_t copy_stream = nullptr; // its H2D copies run here, under the previous batch's kernels
    hipEvent_t ev_copied[2] = {}, ev_consumed[2] = {};
    const uint16_t* cur_input = nullptr;
    musica_contrast_params* d_cparams = nullptr;
    uint32_t* d_plot = nullptr;        // one MUSICA_HIST_RENDER_WIDTH x MUSICA_HIST_RENDER_HEIGHT rgba8 image (the RENDER_HISTS plots, on demand)
    bool fuse_gh;              // the level-0 expand launch accumulates the gradation histogram
    // The expand launches of levels 0 .. 2 compute the 5 x 5 RMS of their band image themselves (k_expand_fast<.., SD>) and the sdev +
    // noise-histogram launches of those levels store nothing: 8 of a step's 48 bytes per input pixel. Whole steps run that way
    // (StepForm::sd_levels); the stage entry points, getters and dumps want the stored images: ensure_sdev() writes them on demand.
    bool sd_fused, sdev_stored = true;
    bool pair_rb_sdev;         // the one-stream script pairs the sdev pass of level i with reduce + band of level i + 1 in one launch (k_rb_sdev); MUSICA_PAIR_RB_SDEV
    bool sdev_one_launch;      // the sdev + noise-histogram passes of levels 0 .. 3 as ONE launch of k_sdev_hist; MUSICA_SDEV_ONE_LAUNCH=0: one launch per marching level + one for the runs
    int rows_rb[MUSICA_MAX_LEVELS];   // its coarse rows per wavefront
    // Level 0's reduce + band launch of a whole-step script counts the level's noise histogram itself (k_reduce_band_hist) and the level-0
    // sdev pass shrinks to the seam columns (StepForm::hist_rows). MUSICA_HIST_IN_RB: 0 never, 1 wherever the form exists, unset (-1):
    // the one-stream steps large enough for segments of 16 coarse rows (hist_rb_rows()).
    int hist_in_rb;
    int hist_rb_rows;          // MUSICA_HIST_RB_ROWS: coarse rows per wavefront of that launch (a multiple of 8), 0: chosen from the step's size
    int xcd_swizzle;           // XCD-aware workgroup -> tile mapping of the marching kernels (launchers.h); MUSICA_XCD_SWIZZLE=0: the plain mapping
    int xcd_regions;           // the metric kernel's 2-D regions per XCD where its geometry allows; MUSICA_XCD_REGIONS=0: the round-3 mapping
    uint8_t* d_out8 = nullptr;   // saveOutImage's cropped 8-bit pixels of one image (device) and their pinned host copy, allocated on first use
    uint8_t* h_out8 = nullptr;
    uint8_t* h_bmp = nullptr;    // saveOutImage's whole file image in page-locked memory: 2 bytes of padding, the 54-byte header, then the pixel array the
                                 // device writes itself (k_out_bmp24: the array starts on a 4-byte boundary); allocated on first use
    StudyState study;        // musica_sim_* / musica_alter_* (musica_study.hip); nothing else reads it, an image lane's copy included
    uint16_t* d_input_kept = nullptr;    // the last step's input when an alteration overwrites d_input after it (the on-demand getters read it)
    // musica_export_out / musica_stream_wait / musica_stream_signal: a step has been enqueued (the export refuses a context without one), and
    // the two events that order the context's stream against a caller's stream, created on first use
    bool stepped = false;
    hipEvent_t ev_caller = nullptr, ev_signal = nullptr;
    // host parameters (src/vk_processing.cpp:259-297, 321-325)
    musica_contrast_params h_cparams[MUSICA_MAX_LEVELS];
    musica_nr_params h_nr[3];
    // rows each wavefront marches per launch, per level (heuristic, then autotuned at create)
    int rows_expand[MUSICA_MAX_LEVELS], rows_sdev[4];
    // tunables
    int expand_rows, sdev_rows, grad_groups;
    // profiling
    uint32_t profiling = 0;  // bit i set: bracket kernel family i with HIP events
    std::vector<ProfSpan> spans;
    size_t spans_used = 0;
    double prof_total_us[MUSICA_KERNEL_COUNT] = {};
    uint64_t prof_count[MUSICA_KERNEL_COUNT] = {};
    bool needs_reset = false;  // a step failed (launch / sync error): the self-resetting tickets of k_minmax_u16 and k_grad_recount_curve may hold a
                               // partial count, which would leave every later launch without a last-ticket block — zeroed before the next step
    std::vector<void*> allocations;
    // Image lanes (musica_execute of a context with a batch, from page-locked host memory): shallow copies of the context for one or
    // two images each — device pointers moved to those images — whose one-stream script is enqueued behind the host-to-device copy of
    // just those images. Every stage of the path is per image, so nothing changes in the results; the first images' kernels run under
    // the remaining copies. Created on first use.
    std::vector<musica_ctx*> lanes;
    hipStream_t lane_stream[kLaneStreams] = {};
    hipStream_t lane_copy[2] = {};   // the images' copies ([1]: unused; two alternating copy streams made every copy twice as long)
    hipEvent_t lane_done[kLaneStreams] = {}, lane_start = nullptr;
    std::vector<hipEvent_t> img_copied;   // one per image
};

// Calls f(member, elements per image) for every member of DeviceBuffers, in allocation order; 0 elements: a buffer this context does
// not have. Returns the number of pointers visited (create_impl checks it against the size of DeviceBuffers).
template <typename D, typename F>
static size_t for_each_buffer(D& d, const musica_ctx& c, F f) {
    size_t visited = 0;
    auto v = [&](auto& ptr, size_t count) { f(ptr, count); visited++; };
    const bool clahe = (c.p.flags & MUSICA_FLAG_CLAHE) != 0;
    const size_t plane0 = c.lv[0].plane, tiles = (size_t)MUSICA_CLAHE_TILES * MUSICA_CLAHE_TILES * MUSICA_CLAHE_BINS;
    v(d.d_input, (size_t)c.N * c.N);
    v(d.d_minmax, kMinMaxStride);
    v(d.d_mm_slots, kMinMaxSlots);
    v(d.d_mm_ticket, kMinMaxStride);   // one 128-byte line per image
    v(d.d_gr_ticket, kGradTicketStride);
    v(d.d_norm, plane0);
    for (int i = 0; i < MUSICA_MAX_LEVELS; i++) {
        v(d.d_down[i], i < c.L ? c.lv[i + 1].plane : 0);
        v(d.d_band[i], i < c.L ? c.lv[i].plane : 0);
        v(d.d_recon[i], i < c.L ? c.lv[i].plane : 0);
        if (i <= MUSICA_CNR_LEVEL) v(d.d_sdev[i], i < c.L ? c.lv[i].plane : 0);
    }
    v(d.d_noise_hist, 4 * MUSICA_NOISE_BINS);
    v(d.d_noise_max, c.L);
    v(d.d_curves, c.L);
    v(d.d_luts, MUSICA_COARSER_LEVELS_START);
    v(d.d_cnr, c.lv[MUSICA_CNR_LEVEL].plane);
    v(d.d_grad_hist, MUSICA_GRAD_BINS);
    v(d.d_grad_hist_b, MUSICA_GRAD_BINS);
    v(d.d_gzero, 1);
    v(d.d_thr090, 1);
    v(d.d_stats_partial, kStatsMaxBlocks);
    v(d.d_le090, c.fuse_gh ? (size_t)c.lv[1].S * (c.lv[0].S / 8) : 0);
    v(d.d_grad_max, 1);
    v(d.d_gcurve, 1);
    v(d.d_graded, plane0);
    v(d.d_scratch, plane0);
    v(d.d_stats, 1);
    v(d.d_clahe_hist, clahe ? tiles : 0);
    v(d.d_clahe_pts, clahe ? tiles : 0);
    v(d.d_clahe_graded, clahe ? plane0 : 0);
    return visited;
}
// Elements per image of `buf`, a member of c's DeviceBuffers, and image idx's slice of it.
template <typename T>
static size_t per_image(const musica_ctx* c, T* const& buf) {
    size_t count = 0;
    for_each_buffer(*c, *c, [&](auto& ptr, size_t n) { if ((const void*)&ptr == (const void*)&buf) count = n; });
    return count;
}
template <typename T>
static T* image_slice(const musica_ctx* c, T* const& buf, uint32_t idx) { return buf + (size_t)idx * per_image(c, buf); }

template <typename T>
static bool dalloc(musica_ctx* c, T** out, size_t count) {
    void* p = nullptr;
    if (count == 0) count = 1;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) return false;
    // "never-written texels read as 0" (Q2). hipMemset runs on the null stream, which the context's non-blocking streams do not wait for:
    // drain it here, or a buffer allocated on first use (the 8-bit output, the second input buffer) could be zeroed AFTER the first
    // kernel or copy has written it (seen once as zero rows at the top of saveOutImage's pixels)
    if (hipMemset(p, 0, count * sizeof(T)) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) { hipFree(p); return false; }
    c->allocations.push_back(p);
    *out = (T*)p;
    return true;
}

// A buffer allocated on first use: true when *out is there, allocated and zeroed now if it was not.
template <typename T>
static bool ensure(musica_ctx* c, T** out, size_t count) { return *out || dalloc(c, out, count); }

// Gives a dalloc'ed buffer (or none) back once the context's stream has drained: work enqueued there may still use it.
template <typename T>
static hipError_t drelease(musica_ctx* c, T** buf) {
    if (!*buf) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    c->allocations.erase(std::remove(c->allocations.begin(), c->allocations.end(), (void*)*buf), c->allocations.end());
    hipFree(*buf);
    *buf = nullptr;
    return hipSuccess;
}

// ---- the step (musica_step.hip) ----------------------------------------------------------------------------------------------
// The form of the launches about to be enqueued: computed by step_form() at the top of whatever enqueues, never kept on the context
// (rows_sdev changes under autotune, copy_rows and the image lanes).
enum StepPurpose {
    STEP_WHOLE,      // a whole step: the scripts, graph capture
    STEP_STAGE,      // a single stage, ensure_sdev, the getters: one launch per level and stage, every sdev image stored and read
    STEP_AUTOTUNE,   // the launches autotune times: a whole step's without the histogram-counting level-0 launch
};
struct StepForm {
    uint32_t sd_levels = 0;   // bit i: level i's expand launch computes its sdev image itself, which this step neither stores nor reads
    int hist_rows = 0;        // coarse rows per wavefront of the level-0 reduce + band launch that counts the noise histogram, 0: it does not
    int tail;                 // the first level of the tiny tail, L: none
    int pairs = 0;            // launches that pair level i's sdev pass with reduce + band of level i + 1 (one stream only)
    bool sdev_one;            // the sdev passes still to run behind the pairs and the seam are one launch, else ...
    int merged;               // ... one launch per level below this one and one for the 16-row-run levels from it on
    bool sd(int i) const { return (sd_levels >> i) & 1u; }
};
HIDDEN StepForm step_form(const musica_ctx* c, StepPurpose purpose);
HIDDEN bool rb_level(const musica_ctx* c, int i);
// Launch geometry of a step of `batch` images before autotune: rows per wavefront of the expand, sdev and reduce + band launches
// (results never depend on it); autotune() times candidates at create, copy_rows() hands its choice to an identical context.
HIDDEN void default_rows(musica_ctx* c, int batch);
HIDDEN void autotune(musica_ctx* c);
HIDDEN void copy_rows(musica_ctx* dst, const musica_ctx* src);
HIDDEN void collect_spans(musica_ctx* c);
// The normalized image / the stored sdev images of levels whose hot path does not store them (getters, dumps, stage entry points).
HIDDEN void ensure_normalized(musica_ctx* c);
HIDDEN void ensure_sdev(musica_ctx* c);
HIDDEN ExpandArgs expand_args(musica_ctx* c, const StepForm& f, int lvl, float* dst);
static inline uint32_t cnr_scale(int S, int cnrS) { return (uint32_t)ceilf((float)S / (float)cnrS); }  // noise_reduction.comp:38
static inline int gain_mode(int lvl) { return lvl > MUSICA_CNR_LEVEL ? GAIN_CONST : (lvl == MUSICA_CNR_LEVEL ? GAIN_RANGE : GAIN_CURVE); }
static inline bool uses_nr(int lvl) { return lvl < MUSICA_CNR_LEVEL - 1; }  // currentLevel < cnrLevel - 1, src/vk_processing.cpp:1009-1016

#define CHECK_CTX(c) do { if (!(c)) return fail("%s: ctx is NULL", __func__); if (hipSetDevice((c)->p.device) != hipSuccess) return fail("%s: hipSetDevice failed", __func__); } while (0)
#define CHECK_IMG(c, idx) do { if ((int)(idx) >= (c)->B) return fail("%s: image_index %u >= batch %d", __func__, (unsigned)(idx), (c)->B); } while (0)
