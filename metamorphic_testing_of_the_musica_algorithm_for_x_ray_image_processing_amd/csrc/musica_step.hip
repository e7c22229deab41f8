// musica_step.hip — one step of the pipeline: the dispatch script that replaces VulkanProcessing::execute (src/vk_processing.cpp:2104-2601
// of the reference). The form a step takes (StepForm), its one launch sequence on one or two streams, graph capture and replay, the launch
// geometry (row heuristics, autotune), the image lanes and the entry points that run a step or a single stage of it.
#include <math.h>
#include <string.h>

#include "musica_ctx.h"

// ---- launch geometry ----------------------------------------------------------------------
void copy_rows(musica_ctx* dst, const musica_ctx* src) {
    if (dst == src) return;
    memcpy(dst->rows_expand, src->rows_expand, sizeof(src->rows_expand));
    memcpy(dst->rows_sdev, src->rows_sdev, sizeof(src->rows_sdev));
    memcpy(dst->rows_rb, src->rows_rb, sizeof(src->rows_rb));
}

// Halves dflt rows per wavefront down to min_rows until the launch has min_waves wavefronts.
static int pick_rows(int dflt, int min_rows, int S, int rows_total, int batch, int min_waves = 2048) {
    int rpw = dflt;
    const int strips = (S + kStripCols - 1) / kStripCols;
    while (rpw > min_rows) {
        const long waves = (long)strips * ((rows_total + rpw - 1) / rpw) * batch;
        if (waves >= min_waves) break;
        rpw /= 2;
    }
    return rpw < min_rows ? min_rows : rpw;
}
// Rows per wavefront of the sdev + noise-histogram launch of level i; 0 = one 16-row run per workgroup (sdev_run_block), the
// form for every launch that cannot fill the chip with 16-row marches (MUSICA_SDEV_RUN=0 / 1: never / always).
static int sdev_rows_default(const musica_ctx* c, int i, int batch) {
    const int mode = env_int("MUSICA_SDEV_RUN", -1);
    // 16-row marches of this launch: with fewer than one per SIMD (1024) each walks its 20 dependent row trips alone (17 - 18 us
    // whatever the size); the run form costs 9 - 13 us there but reads its input twice: slower once the marches fill the chip
    // (8 x 2048^2, every kernel alone: level 0 74.7 against 61.5 us, level 1 27.4 / 23.6, level 2 13.1 / 18.8, level 3 9.9 / 18.1)
    const long marches = (long)((c->lv[i].S + kStripCols - 1) / kStripCols) * ((c->lv[i].S + kHistArea - 1) / kHistArea) * batch;
    if (mode == 1 || (mode < 0 && marches < 1024)) return 0;
    return pick_rows(c->sdev_rows, 16, c->lv[i].S, c->lv[i].S, batch);
}
void default_rows(musica_ctx* c, int batch) {
    for (int i = 0; i < c->L; i++) {
        c->rows_expand[i] = pick_rows(c->expand_rows, 1, c->lv[i].S, c->lv[i + 1].S, batch);
        if (i <= MUSICA_CNR_LEVEL) c->rows_sdev[i] = sdev_rows_default(c, i, batch);
        c->rows_rb[i] = pick_rows(env_int("MUSICA_RB_ROWS", 16), 1, c->lv[i].S, c->lv[i + 1].S, batch);
    }
}

// ---- profiling spans --------------------------------------------------------------------
struct Span {
    musica_ctx* c;
    ProfSpan* s;
    hipStream_t st;
    Span(musica_ctx* ctx, int id) : c(ctx), s(nullptr), st(ctx->cur) {
        if (!((c->profiling >> id) & 1u)) return;
        if (c->spans_used == c->spans.size()) {
            ProfSpan n;
            n.id = id;
            hipEventCreate(&n.a);
            hipEventCreate(&n.b);
            c->spans.push_back(n);
        }
        s = &c->spans[c->spans_used++];
        s->id = id;
        hipEventRecord(s->a, st);
    }
    ~Span() {
        if (s) hipEventRecord(s->b, st);
    }
};

void collect_spans(musica_ctx* c) {
    for (size_t i = 0; i < c->spans_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->spans[i].a, c->spans[i].b) == hipSuccess) {
            c->prof_total_us[c->spans[i].id] += (double)ms * 1000.0;
            c->prof_count[c->spans[i].id] += 1;
        }
    }
    c->spans_used = 0;
}

// ---- the form of a step ---------------------------------------------------------------------
// reduce + band of a level in one launch: every level whose side is a multiple of 8 (level 0 then reads the raw pixels)
bool rb_level(const musica_ctx* c, int i) { return !c->generic && c->lv[i].S >= 8 && (c->lv[i].S % 8) == 0; }
// Coarse rows per wavefront of level 0's launch in the form that counts the noise histogram itself, 0 where the context does not take it.
// A wavefront scans whole 16-row runs of its own segment: 8 k coarse rows (MUSICA_HIST_RB_ROWS sets k). By default the form is taken where
// segments of 16 coarse rows fill the chip and the step runs on one stream (the contexts of a pipeline; the two-stream script of a
// lone context has the level-0 sdev pass beside the reduce tail already, and a longer level-0 launch in front of it: profiles/r07);
// MUSICA_HIST_IN_RB=1 takes it wherever it exists, down to segments of one run.
static int hist_rb_rows(const musica_ctx* c) {
    if (c->hist_in_rb == 0 || c->hist_cov <= 0) return 0;   // a side below 512 lies outside the dispatch coverage: nothing to count
    // 16 coarse rows where that gives every SIMD a wavefront, else 8 (rows_rb[0] is tuned for the launch without the scan, and at init:
    // its choice varies from process to process). Same-box A/B at 8 x 2048^2, three steps in flight: 16 rows -3.4 %, 32 rows -0.6 %.
    const int r = pick_rows(16, 8, c->lv[0].S, c->lv[1].S, c->B, 1024);
    if (c->hist_in_rb < 0 && !(r == 16 && c->dag == 0)) return 0;
    return c->hist_rb_rows > 0 ? c->hist_rb_rows : r;
}
// The first level of the tiny tail (k_tiny_tail: reduce + band of levels T .. L-1 and their expand slots in one launch), L if none:
// levels above the cnr level whose side is at most kTailSide, where there are at least two of them (a lone level is two launches
// either way).
static int tail_first(const musica_ctx* c) {
    if (!c->tiny_tail) return c->L;
    int T = c->L;
    while (T - 1 > MUSICA_CNR_LEVEL && c->lv[T - 1].S <= kTailSide) T--;
    if (c->L - T > kTailMax) T = c->L - kTailMax;
    return c->L - T >= 2 ? T : c->L;
}
// the first level from which every sdev launch is the 16-row-run form (MUSICA_CNR_LEVEL + 1: none)
static int sdev_runs_from(const musica_ctx* c) {
    if (c->ref_order) return MUSICA_CNR_LEVEL + 1;
    int first = MUSICA_CNR_LEVEL + 1;
    while (first > 0 && c->rows_sdev[first - 1] <= 0) first--;
    return first;
}
StepForm step_form(const musica_ctx* c, StepPurpose purpose) {
    StepForm f;
    f.tail = c->L;
    f.sdev_one = c->sdev_one_launch && !c->ref_order;
    if (purpose != STEP_STAGE) {
        // levels below the cnr level whose side takes the streaming kernels
        for (int i = 0; c->sd_fused && i < MUSICA_CNR_LEVEL; i++)
            if (rb_level(c, i)) f.sd_levels |= 1u << i;
        // the autotune pass times the level-0 launch without the scan (rows_rb[0] is its geometry, not the scanning launch's)
        if (purpose == STEP_WHOLE && c->sd_fused && !c->ref_order && !c->generic && c->fuse_u16 && rb_level(c, 0)) f.hist_rows = hist_rb_rows(c);
        f.tail = tail_first(c);
        // the pairs of the one-stream script: level i's sdev pass with reduce + band of level i + 1 for i = 0, 1, .. while both levels take the
        // streaming reduce + band launch and level i + 1 lies above the tiny tail; what is left of the sdev passes is then one launch
        if (c->dag == 0 && c->pair_rb_sdev && !c->ref_order && !c->generic) {
            while (f.pairs <= MUSICA_CNR_LEVEL && f.pairs + 1 < f.tail && rb_level(c, f.pairs) && rb_level(c, f.pairs + 1)) f.pairs++;
            f.sdev_one = true;
        }
    }
    f.merged = std::max(sdev_runs_from(c), f.hist_rows > 0 ? 1 : 0);
    if (f.merged >= MUSICA_CNR_LEVEL) f.merged = MUSICA_CNR_LEVEL + 1;   // one level is its own launch
    return f;
}
// What a whole step leaves behind, eager, replayed or run by the image lanes: the normalized image only where a launch of the step stores
// it, and no sdev image of the levels whose expand launches compute it (ensure_normalized / ensure_sdev write them on demand).
static bool stores_norm(const musica_ctx* c) { return !c->fuse_u16 || (c->d_clahe_hist && !c->clahe_raw); }  // a CLAHE block that reads the stored normalized image through k_relevant
static void step_done(musica_ctx* c) {
    c->norm_valid = stores_norm(c);
    if (c->sd_fused) c->sdev_stored = false;
}

// ---- the launches of a step -------------------------------------------------------------------
constexpr size_t kNoiseHistStride = (size_t)4 * MUSICA_NOISE_BINS;   // u32 per image of d_noise_hist: levels 0 .. 3
static uint32_t* noise_hist_of(const musica_ctx* c, int i) { return c->d_noise_hist + (size_t)i * MUSICA_NOISE_BINS; }
static const float* level_input(musica_ctx* c, int i) { return i == 0 ? c->d_norm : c->d_down[i - 1]; }  // src/vk_processing.cpp:758-761

// stage "norm" (src/vk_processing.cpp:2182-2222)
// with_clears: the launch also zeroes the histograms (src/vk_processing.cpp:2153-2162)
static void enqueue_norm(musica_ctx* c, bool with_clears) {
    {
        Span sp(c, MUSICA_KERNEL_MINMAX);
        if (with_clears) launch_minmax(c->stream, c->cur_input, c->N, c->d_minmax, c->d_mm_slots, c->d_mm_ticket, c->B, c->d_noise_hist, c->d_grad_hist, c->d_grad_hist_b, c->d_gzero, c->d_clahe_hist);
        else launch_minmax(c->stream, c->cur_input, c->N, c->d_minmax, c->d_mm_slots, c->d_mm_ticket, c->B);
    }
    c->norm_valid = false;
    if (stores_norm(c)) {
        Span sp(c, MUSICA_KERNEL_NORMALIZE);
        launch_normalize(c->stream, c->cur_input, c->d_norm, c->lv[0], c->d_minmax, c->min_chain_exact, c->B);
        c->norm_valid = true;
    }
}
void ensure_normalized(musica_ctx* c) {
    if (c->norm_valid) return;
    launch_normalize(c->stream, c->cur_input, c->d_norm, c->lv[0], c->d_minmax, c->min_chain_exact, c->B);
    c->norm_valid = true;
}

static void run_reduce_band(musica_ctx* c, const StepForm& f, int i, int rows) {
    if (i == 0 && f.hist_rows > 0)
        launch_reduce_band_u16_hist(c->cur, c->cur_input, c->d_down[0], c->d_band[0], c->lv[0], c->lv[1], c->B, f.hist_rows, c->d_minmax, c->min_chain_exact,
                                    c->d_le090, c->xcd_swizzle, noise_hist_of(c, 0), kNoiseHistStride, c->hist_cov);
    else if (i == 0)
        launch_reduce_band_u16(c->cur, c->cur_input, c->d_down[0], c->d_band[0], c->lv[0], c->lv[1], c->B, rows, c->d_minmax, c->min_chain_exact, c->d_le090,
                               c->xcd_swizzle);
    else
        launch_reduce_band(c->cur, level_input(c, i), c->d_down[i], c->d_band[i], c->lv[i], c->lv[i + 1], c->B, rows, c->xcd_swizzle);
}
// reduce and band of level i, as one launch where that form applies, else the one-thread-per-texel kernels
static void run_reduce_and_band(musica_ctx* c, const StepForm& f, int i) {
    if (rb_level(c, i)) { Span sp(c, i == 0 ? MUSICA_KERNEL_REDUCE_L0 : MUSICA_KERNEL_REDUCE_REST); run_reduce_band(c, f, i, c->rows_rb[i]); return; }
    { Span sp(c, i == 0 ? MUSICA_KERNEL_REDUCE_L0 : MUSICA_KERNEL_REDUCE_REST); launch_reduce(c->cur, level_input(c, i), c->lv[i], c->d_down[i], c->lv[i + 1], c->B, true, i == 0 ? 0 : 1, c->xcd_swizzle, c->xcd_regions, c->ref_order); }
    { Span sp(c, i == 0 ? MUSICA_KERNEL_BAND_L0 : MUSICA_KERNEL_BAND_REST); launch_band(c->cur, level_input(c, i), c->d_down[i], c->d_band[i], c->lv[i], c->lv[i + 1], c->B, c->ref_order); }
}
static void run_tiny_tail(musica_ctx* c, int T) {
    TailArgs a;
    a.n = c->L - T;
    for (int k = 0; k < a.n; k++) {
        const int i = T + k;
        a.l[k] = TailLevel{level_input(c, i), c->d_down[i], c->d_band[i], c->d_recon[i], c->lv[i].plane, c->lv[i].S, c->lv[i].pitch,
                           c->h_cparams[i].highContrastFactor};
    }
    for (int k = a.n; k < kTailMax; k++) a.l[k] = a.l[0];
    a.Sl = c->lv[c->L].S; a.lpitch = c->lv[c->L].pitch; a.lplane = c->lv[c->L].plane;
    a.ref = c->ref_order;
    Span sp(c, MUSICA_KERNEL_REDUCE_REST);
    launch_tiny_tail(c->cur, a, c->B);
}
// stage "red" (src/vk_processing.cpp:2233-2273): reduce + band of levels first .. end - 1, the levels of the tiny tail (with their expand
// slots) in its one launch
static void enqueue_reduce(musica_ctx* c, const StepForm& f, int first, int end) {
    for (int i = first; i < end && i < f.tail; i++) run_reduce_and_band(c, f, i);
    if (end > f.tail) run_tiny_tail(c, f.tail);
}

// stage "anly" (src/vk_processing.cpp:2284-2357)
// the fast order's sdev images of the levels whose hot path does not store them (no histogram), for getters / dumps / the stage entry points
void ensure_sdev(musica_ctx* c) {
    if (c->sdev_stored) return;
    const int rows = 16;
    for (int i = 0; i < MUSICA_CNR_LEVEL && i < c->L; i++)
        if (rb_level(c, i)) launch_sdev_hist(c->stream, 1, &c->d_band[i], &c->d_sdev[i], &c->lv[i], nullptr, &rows, 0, 0, c->B, c->xcd_swizzle);
    c->sdev_stored = true;
}
// The sdev + noise-histogram passes of levels first .. last as ONE launch (k_sdev_hist: they depend on nothing but their own band image), every
// level in the form rows_sdev gives it, or all of them in the form of `rows` where that is >= 0 (autotune's candidates). Under
// MUSICA_FLAG_REFERENCE_ORDER a level at a time: img_sdev.comp literally, then noise_hist.comp on the stored image.
static void run_sdev_levels(musica_ctx* c, const StepForm& f, int first, int last, int rows = -1) {
    if (c->ref_order) {
        for (int i = first; i <= last; i++) {
            Span sp(c, MUSICA_KERNEL_SDEV_HIST);
            launch_sdev_literal(c->cur, c->d_band[i], c->d_sdev[i], c->lv[i], c->B);
            launch_noise_hist_only(c->cur, c->d_sdev[i], c->lv[i], noise_hist_of(c, i), kNoiseHistStride, c->hist_cov, c->B);
        }
        return;
    }
    float* sdev[kSdevRunLevelsMax];
    uint32_t* hist[kSdevRunLevelsMax];
    int rws[kSdevRunLevelsMax];
    const int n = last - first + 1;
    for (int k = 0; k < n; k++) {
        sdev[k] = f.sd(first + k) ? nullptr : c->d_sdev[first + k];
        hist[k] = noise_hist_of(c, first + k);
        rws[k] = rows >= 0 ? rows : c->rows_sdev[first + k];
    }
    Span sp(c, MUSICA_KERNEL_SDEV_HIST);
    launch_sdev_hist(c->cur, n, &c->d_band[first], sdev, &c->lv[first], hist, rws, kNoiseHistStride, c->hist_cov, c->B, c->xcd_swizzle);
}
// The sdev + noise-histogram passes still to run from level i on. Where level 0's histogram came out of its reduce + band launch, the seam
// columns are what is left of its pass (a launch of its own here; a pair runs it in the sdev role). Then one launch, or one per marching
// level and one for the runs (i < coarserLevelsStart || i <= cnrLevel, :2285).
static void enqueue_sdev_from(musica_ctx* c, const StepForm& f, int i) {
    if (i == 0 && f.hist_rows > 0) {
        Span sp(c, MUSICA_KERNEL_SDEV_HIST);
        launch_hist_seam(c->cur, c->d_band[0], c->lv[0], noise_hist_of(c, 0), kNoiseHistStride, c->hist_cov, c->B);
        i = 1;
    }
    if (i > MUSICA_CNR_LEVEL) return;
    if (f.sdev_one) { run_sdev_levels(c, f, i, MUSICA_CNR_LEVEL); return; }
    for (; i < f.merged; i++) run_sdev_levels(c, f, i, i);
    if (i <= MUSICA_CNR_LEVEL) run_sdev_levels(c, f, i, MUSICA_CNR_LEVEL);   // the levels from f.merged on all take the run form
}
// curves of every level + cnr of level 3 in one launch (kernels_analysis.hip k_curves_cnr)
static void run_curves_cnr(musica_ctx* c) {
    Span sp(c, MUSICA_KERNEL_CURVES);
    launch_curves_cnr(c->cur, c->d_noise_hist, kNoiseHistStride, c->d_noise_max, c->d_curves, c->d_cparams, c->L, c->B, c->d_luts,
                      c->d_sdev[MUSICA_CNR_LEVEL], c->d_cnr, c->lv[MUSICA_CNR_LEVEL], c->d_minmax, c->min_chain_exact, c->d_thr090);
}
// reduce + band of level i + 1 and the sdev + noise-histogram pass of level i as one launch (k_rb_sdev): both wait for reduce + band of level i only
static void run_rb_sdev_pair(musica_ctx* c, const StepForm& f, int i) {
    const int r = i + 1;
    RbSdevArgs a;
    a.fine = level_input(c, r); a.down = c->d_down[r]; a.band = c->d_band[r];
    a.S = c->lv[r].S; a.pitch = c->lv[r].pitch; a.plane = c->lv[r].plane;
    a.Sc = c->lv[r + 1].S; a.cpitch = c->lv[r + 1].pitch; a.cplane = c->lv[r + 1].plane;
    a.rows_rb = c->rows_rb[r];
    a.sl.band = c->d_band[i]; a.sl.sdev = f.sd(i) ? nullptr : c->d_sdev[i];
    a.sl.hist = noise_hist_of(c, i);
    a.sl.rows = c->rows_sdev[i] > 0 ? c->rows_sdev[i] : 0;
    if (i == 0 && f.hist_rows > 0) a.sl.rows = -1;   // the seam pass in the sdev role
    a.hist_stride = kNoiseHistStride; a.cov = c->hist_cov; a.swz = c->xcd_swizzle;
    Span sp(c, MUSICA_KERNEL_SDEV_HIST);
    launch_rb_sdev(c->cur, a, c->lv[i], c->B);
}

ExpandArgs expand_args(musica_ctx* c, const StepForm& f, int lvl, float* dst) {
    const LevelDesc& lf = c->lv[lvl];
    const LevelDesc& lc = c->lv[lvl + 1];
    const LevelDesc& l3 = c->lv[MUSICA_CNR_LEVEL];
    ExpandArgs a;
    a.prev = lvl == c->L - 1 ? c->d_down[c->L - 1] : c->d_recon[lvl + 1];  // src/vk_processing.cpp:930-934
    a.band = c->d_band[lvl];
    a.sdev = lvl <= MUSICA_CNR_LEVEL && !f.sd(lvl) ? c->d_sdev[lvl] : nullptr;
    a.cnr = c->d_cnr;
    a.recon = dst;
    a.curves = c->d_curves + lvl;
    a.luts = c->d_luts + (lvl < MUSICA_COARSER_LEVELS_START ? lvl : 0);
    a.curve_stride = (size_t)c->L;
    a.S = lf.S; a.pitch = lf.pitch; a.plane = lf.plane;
    a.Sc = lc.S; a.cpitch = lc.pitch; a.cplane = lc.plane;
    a.cnrS = l3.S; a.cnrPitch = l3.pitch; a.cnrPlane = l3.plane;
    a.cnrScale = (int)cnr_scale(lf.S, l3.S);
    a.high = c->h_cparams[lvl].highContrastFactor;
    const musica_nr_params& q = c->h_nr[lvl < 3 ? lvl : 0];
    a.lowCnr = q.lowCnr; a.lowFactor = q.lowFactor; a.highCnr = q.highCnr; a.highFactor = q.highFactor;
    a.rows_per_wave = c->rows_expand[lvl];
    a.raw = nullptr; a.ghist = nullptr; a.gzero = nullptr; a.thr090 = nullptr; a.le090 = nullptr; a.chist = nullptr;
    a.swz = c->xcd_swizzle;
    a.ref_order = c->ref_order;
    return a;
}

// CLAHE contexts: the level-0 expand launch (rows_per_wave = rows) can also count the CLAHE histogram (k_expand_fast<.., CH>): it has
// the `normalized <= 0.9` bits, and a workgroup's 512 columns x 8 * rows rows touch at most 2 x 2 of the 4 x 4 tiles
static bool clahe_hist_in_expand(const musica_ctx* c, int rows) {
    const int G = c->lv[0].S / MUSICA_CLAHE_TILES;
    return c->d_clahe_hist && c->clahe_raw && c->fuse_gh && !c->generic && c->d_le090 && c->clahe_in_expand && (c->lv[0].S % MUSICA_CLAHE_TILES) == 0 &&
           G >= 512 && 8 * rows <= G;
}
// with_hist: the level-0 launch of a fusing context also accumulates the gradation histogram (enqueue_gradation(c, true) must follow)
static void run_expand_level(musica_ctx* c, const StepForm& f, int lvl, int rows, bool with_hist) {
    ExpandArgs a = expand_args(c, f, lvl, c->d_recon[lvl]);
    a.rows_per_wave = rows;
    if (with_hist && lvl == 0 && c->fuse_gh && !c->generic) {
        a.raw = c->cur_input; a.ghist = c->d_grad_hist; a.gzero = c->d_gzero; a.thr090 = c->d_thr090;
        a.le090 = c->d_le090;
        if (clahe_hist_in_expand(c, rows)) a.chist = c->d_clahe_hist;
    }
    launch_expand(c->cur, a, gain_mode(lvl), uses_nr(lvl), c->B, c->generic);
}
// stages "aply" + "exp" (src/vk_processing.cpp:2361-2431): the expand slots of levels top down to bottom
static void enqueue_expand(musica_ctx* c, const StepForm& f, int top, int bottom, bool with_hist) {
    for (int lvl = top; lvl >= bottom; lvl--) {
        Span sp(c, lvl == 0 ? MUSICA_KERNEL_EXPAND_L0 : MUSICA_KERNEL_EXPAND_REST);
        run_expand_level(c, f, lvl, c->rows_expand[lvl], with_hist);
    }
}

// stage "grad" (src/vk_processing.cpp:2456-2518)
// fused: the level-0 expand launch has already accumulated the histogram (run_expand_level with_hist); what is left of K18 + K19 is
// the literal recount of images that hold an exact zero (a launch that returns at once for every other image).
static void enqueue_gradation(musica_ctx* c, bool fused) {
    fused = fused && c->fuse_gh && !c->generic;
    const LevelDesc& l0 = c->lv[0];
    const LevelDesc& l3 = c->lv[MUSICA_CNR_LEVEL];
    const int scale = (int)cnr_scale(l0.S, l3.S);
    const bool ch_done = fused && clahe_hist_in_expand(c, c->rows_expand[0]);   // the level-0 expand launch counted the CLAHE histogram
    const bool one_apply = c->d_clahe_hist && c->clahe_raw && !c->generic && (l0.S % 4) == 0 && c->clahe_one_apply;   // both curves in one pass
    if (c->d_clahe_hist) {  // #ifdef ENABLE_CLAHE block, src/vk_processing.cpp:2471-2489
        hipStream_t cs = c->stream;
        if (c->clahe_raw) {   // relevance computed inside the histogram launch from the raw pixels: no relevant image on the hot path
            launch_clahe(cs, c->d_recon[0], nullptr, c->d_clahe_graded, l0, c->d_clahe_hist, c->d_clahe_pts, c->B, c->cur_input, c->d_thr090, c->d_cnr, &l3, scale,
                         ch_done, !one_apply);
        } else {
            launch_relevant(cs, c->d_norm, c->d_cnr, c->d_scratch, l0, l3, scale, c->B);
            launch_clahe(cs, c->d_recon[0], c->d_scratch, c->d_clahe_graded, l0, c->d_clahe_hist, c->d_clahe_pts, c->B);
        }
    }
    GradArgs g;
    g.img = c->d_recon[0]; g.normalized = c->d_norm; g.cnr = c->d_cnr; g.hist = fused ? c->d_grad_hist_b : c->d_grad_hist;
    g.only_if = fused ? c->d_gzero : nullptr;
    g.N = l0.S; g.pitch = l0.pitch; g.plane = l0.plane;
    g.cnrS = l3.S; g.cnrPitch = l3.pitch; g.cnrPlane = l3.plane; g.cnrScale = scale;
    g.groups_per_wave = c->grad_groups;
    g.raw = c->fuse_u16 ? c->cur_input : nullptr;
    g.minmax = c->d_minmax;
    g.min_chain_exact = c->min_chain_exact;
    if (fused && c->grad_one_launch) {   // the recount of images that hold an exact zero and the tone curve in one launch
        Span sp(c, MUSICA_KERNEL_GRAD_CURVE);
        launch_grad_recount_curve(c->stream, g, c->d_grad_hist, c->d_grad_max, c->d_gcurve, c->d_gr_ticket, c->B);
    } else {
        { Span sp(c, MUSICA_KERNEL_GRAD_HIST); launch_grad_hist(c->stream, g, c->B); }
        Span sp(c, MUSICA_KERNEL_GRAD_CURVE);
        launch_grad_curve(c->stream, c->d_grad_hist, c->d_grad_max, c->d_gcurve, c->B, fused ? c->d_grad_hist_b : nullptr, fused ? c->d_gzero : nullptr);
    }
    if (one_apply) {
        Span sp(c, MUSICA_KERNEL_GRAD_APPLY);
        launch_grad_clahe_apply(c->stream, c->d_recon[0], c->d_clahe_graded, c->d_graded, l0, c->d_clahe_pts, c->d_gcurve, c->B);
        return;
    }
    { Span sp(c, MUSICA_KERNEL_GRAD_APPLY); launch_grad_apply(c->stream, c->d_recon[0], c->d_graded, l0, c->d_gcurve, c->B); }
}

// ---- the launch sequence ----------------------------------------------------------------------
// One in-order stream, the order of the reference's command buffer (dag == 0), with f.pairs >= 0 of the launches that pair level i's sdev
// pass with reduce + band of level i + 1: minmax RB0 [RB1 | S0] [RB2 | S1] [RB3 | S2] [RB4 | S3] RB5 .. [tail] curves+cnr E .. gradation —
// the pyramid's dependent chain of ever smaller launches in the shadow of the sdev passes instead of in front of them.
static void enqueue_one_stream(musica_ctx* c, const StepForm& f) {
    c->cur = c->stream;
    enqueue_norm(c, true);   // with the clears of :2153-2162
    run_reduce_and_band(c, f, 0);
    for (int i = 0; i < f.pairs; i++) run_rb_sdev_pair(c, f, i);
    enqueue_reduce(c, f, f.pairs + 1, c->L);
    enqueue_sdev_from(c, f, f.pairs);
    run_curves_cnr(c);
    enqueue_expand(c, f, f.tail - 1, 0, true);
    enqueue_gradation(c, true);
}
// Two streams, one fork and one join (dag == 2): the analysis (the sdev + noise-histogram launches and the curves: they read band 0 .. 3
// and nothing of the levels above) runs on the side stream BESIDE the tail of the reduce chain and the constant-gain expand slots
// (levels >= 4 down to expand 3: launches of a few microseconds each that read nothing the analysis writes).
//   stream : minmax RB0 RB1 RB2 RB3 | RB4 .. RB(L-1) E(L-1) .. E3 | (wait) E2 E1 E0 gradation
//   side   :                        | S(0..3) curves+cnr          |
static void enqueue_two_streams(musica_ctx* c, const StepForm& f) {
    c->cur = c->stream;
    enqueue_norm(c, true);
    enqueue_reduce(c, f, 0, MUSICA_CNR_LEVEL + 1);
    hipEventRecord(c->ev_fork, c->stream);
    hipStreamWaitEvent(c->side, c->ev_fork, 0);
    c->cur = c->side;
    enqueue_sdev_from(c, f, 0);
    run_curves_cnr(c);
    hipEventRecord(c->ev_join, c->side);
    c->cur = c->stream;
    enqueue_reduce(c, f, MUSICA_CNR_LEVEL + 1, c->L);
    enqueue_expand(c, f, f.tail - 1, MUSICA_CNR_LEVEL, true);
    hipStreamWaitEvent(c->stream, c->ev_join, 0);
    enqueue_expand(c, f, MUSICA_CNR_LEVEL - 1, 0, true);
    enqueue_gradation(c, true);
}
static void enqueue_step(musica_ctx* c) {
    const StepForm f = step_form(c, STEP_WHOLE);
    if (c->dag) enqueue_two_streams(c, f);
    else enqueue_one_stream(c, f);
    step_done(c);
}

// Captures the step (with two streams the side stream joins the capture through ev_fork and rejoins
// through ev_join) into an executable graph for the current input pointer.
static int capture_graph(musica_ctx* c) {
    int k = 0;   // an empty slot, else the least recently used one
    for (int j = 0; j < kGraphSlots; j++) {
        if (!c->graph_exec[j]) { k = j; break; }
        if (c->graph_used[j] < c->graph_used[k]) k = j;
    }
    if (c->graph_exec[k]) {
        // its last launch may still be running (musica_execute_device / musica_pipeline_step never wait): drain the stream before
        // the executable graph goes away. Only callers that rotate more than kGraphSlots input pointers ever get here.
        if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
        hipGraphExecDestroy(c->graph_exec[k]);
        c->graph_exec[k] = nullptr; c->graph_input[k] = nullptr;
    }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return -1;
    enqueue_step(c);
    if (hipStreamEndCapture(c->stream, &graph) != hipSuccess || !graph) { (void)hipGetLastError(); return -1; }
    const hipError_t e = hipGraphInstantiate(&c->graph_exec[k], graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) { c->graph_exec[k] = nullptr; (void)hipGetLastError(); return -1; }
    c->graph_input[k] = c->cur_input;
    return k;
}

static void reset_tickets_if_needed(musica_ctx* c) {
    if (!c->needs_reset) return;
    hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    hipMemsetAsync(c->d_mm_ticket, 0, c->B * per_image(c, c->d_mm_ticket) * sizeof(uint32_t), c->stream);
    hipMemsetAsync(c->d_gr_ticket, 0, c->B * per_image(c, c->d_gr_ticket) * sizeof(uint32_t), c->stream);
    c->needs_reset = false;
}
static int enqueue_all_impl(musica_ctx* c);
static int enqueue_all(musica_ctx* c) {
    reset_tickets_if_needed(c);
    const int ok = enqueue_all_impl(c);
    if (!ok) c->needs_reset = true;
    return ok;
}
static int enqueue_all_impl(musica_ctx* c) {
    if (c->use_graph && c->profiling == 0) {
        int k = -1;
        for (int j = 0; j < kGraphSlots; j++)
            if (c->graph_exec[j] && c->graph_input[j] == c->cur_input) { k = j; break; }
        if (k < 0) {
            k = capture_graph(c);
            if (k < 0) c->use_graph = false;   // e.g. a runtime without capture support: stay eager
        }
        if (k >= 0) {
            c->graph_used[k] = ++c->graph_clock;
            step_done(c);
            if (hipGraphLaunch(c->graph_exec[k], c->stream) != hipSuccess) return fail("hipGraphLaunch failed: %s", hipGetErrorString(hipGetLastError()));
            return 1;
        }
    }
    enqueue_step(c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(e));
    return 1;
}

// ---- init-time autotune ------------------------------------------------------------------
// How many rows a wavefront marches decides both the number of wavefronts and the halo re-reads;
// the best value depends on level size, batch and how the workgroups spread over the 8 XCDs, and
// no closed form predicted it on MI355X ("Launch geometry"). So musica_create runs the
// pipeline once on a synthetic input and then times each streaming kernel of every large level for
// a handful of candidates with HIP events, keeping the fastest. Results are independent of the
// choice (the kernels are bit-identical for every row count); only the speed changes.
static float time_launches(musica_ctx* c, hipEvent_t a, hipEvent_t b, int reps, const StepForm& f, void (*fn)(musica_ctx*, const StepForm&, int, int), int level, int rows) {
    fn(c, f, level, rows);  // warm
    float best = 1e30f;
    for (int r = 0; r < reps; r++) {
        hipEventRecord(a, c->stream);
        fn(c, f, level, rows);
        fn(c, f, level, rows);
        hipEventRecord(b, c->stream);
        hipEventSynchronize(b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess && ms < best) best = ms;
    }
    return best;
}

void autotune(musica_ctx* c) {
    const size_t n = (size_t)c->B * c->N * c->N;
    std::vector<uint16_t> px(n);
    uint32_t h = 12345u;
    for (int b = 0; b < c->B; b++)
        for (int y = 0; y < c->N; y++)
            for (int x = 0; x < c->N; x++) {
                h = h * 1664525u + 1013904223u;
                const float base = 20000.0f + 12000.0f * sinf(0.011f * x + b) * cosf(0.007f * y) + ((x / 97 + y / 61) & 1) * 6000.0f;
                const float noise = (float)((h >> 9) & 0xFFFF) / 65536.0f - 0.5f;
                px[((size_t)b * c->N + y) * c->N + x] = (uint16_t)fminf(65535.0f, fmaxf(1.0f, base + 2.0f * sqrtf(base) * noise));
            }
    if (hipMemcpy(c->d_input, px.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) return;
    c->cur_input = c->d_input;
    c->cur = c->stream;
    // Kept as it is, not measured: on a graph-replaying context this warm-up step captures the graph of d_input with the rows chosen before
    // the tuning below, and nothing recaptures it, so later steps on the context's own input buffer replay the untuned geometry (context 0
    // of a pipeline too; the others get copy_rows before their first capture). Changing it changes speed: a matter for a measured change.
    if (!enqueue_all(c)) return;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    const StepForm f = step_form(c, STEP_AUTOTUNE);   // the launches a whole step runs; none of them reads the rows tuned here from the form
    const int reps = 3;
    static const int cand_pair[] = {2, 4, 8, 16};   // band / expand count coarse rows (two fine rows each)
    static const int cand_sdev[] = {0, 16, 32, 64};   // 0: one run per workgroup
    for (int i = 0; i < c->L; i++) {
        if (c->lv[i].S < 512 || (c->lv[i].S % 8) != 0) continue;   // small levels are launch-bound: keep the heuristic
        static const int cand_rb[] = {4, 8, 16, 32, 64};
        struct { int* slot; const int* cand; int ncand; void (*fn)(musica_ctx*, const StepForm&, int, int); bool use; } jobs[3] = {
            {&c->rows_rb[i], cand_rb, 5, run_reduce_band, rb_level(c, i)},
            {&c->rows_expand[i], cand_pair, 4, [](musica_ctx* x, const StepForm& g, int l, int r) { run_expand_level(x, g, l, r, true); }, true},
            {i <= MUSICA_CNR_LEVEL ? &c->rows_sdev[i] : nullptr, cand_sdev, 4, [](musica_ctx* x, const StepForm& g, int l, int r) { run_sdev_levels(x, g, l, l, r > 0 ? r : 0); }, i <= MUSICA_CNR_LEVEL},
        };
        for (auto& j : jobs) {
            if (!j.use) continue;
            float best = time_launches(c, a, b, reps, f, j.fn, i, *j.slot);
            for (int k = 0; k < j.ncand; k++) {
                if (j.cand[k] == *j.slot) continue;
                const float t = time_launches(c, a, b, reps, f, j.fn, i, j.cand[k]);
                if (t < best * 0.97f) { best = t; *j.slot = j.cand[k]; }   // 3 % hysteresis against timer noise
            }
        }
    }
    hipEventDestroy(a);
    hipEventDestroy(b);
    hipStreamSynchronize(c->stream);
}

extern "C" {

// ---- image lanes (see musica_ctx::lanes) ----------------------------------------------------------------------------------
// Shallow copy of the context restricted to image i0: same buffers, every per-image pointer moved to that image, batch 1, one stream,
// its script replayed as a graph of its own.
static musica_ctx* make_lane(const musica_ctx* c, int i0, int nb) {
    musica_ctx* v = new musica_ctx(*c);
    v->allocations.clear();   // the parent owns the memory, the streams and the events
    v->spans.clear();
    v->spans_used = 0;
    v->lanes.clear();
    v->img_copied.clear();
    v->side = nullptr; v->ev_fork = nullptr; v->ev_join = nullptr; v->copy_stream = nullptr;
    v->ev_caller = nullptr; v->ev_signal = nullptr;
    for (int k = 0; k < kGraphSlots; k++) { v->graph_exec[k] = nullptr; v->graph_input[k] = nullptr; v->graph_used[k] = 0; }
    v->use_graph = !(c->p.flags & MUSICA_FLAG_NO_GRAPH) && env_int("MUSICA_GRAPH", 1) != 0;   // one graph per lane and input buffer: the host
                                                                                             // enqueues 8 replays per batch instead of ~136 launches
    v->dag = 0;
    v->profiling = 0;
    v->B = nb;
    v->p.batch = (uint32_t)nb;
    const size_t o = (size_t)i0;
    for_each_buffer(*v, *c, [o](auto& ptr, size_t count) { ptr += o * count; });
    v->cur_input = v->d_input;
    default_rows(v, nb);   // launch geometry of a step of nb images
    return v;
}
// Only for page-locked host memory (musica_host_alloc, hipHostMalloc, hipHostRegister): a copy from pageable memory is staged by the
// runtime and blocks the host meanwhile, so eight of them in a row are slower than one (8 x 2048^2: 2.5 ms against 1.7 ms per batch).
static bool lanes_wanted(const musica_ctx* c, const void* host_pixels) {
    if (!(c->B > 1 && c->profiling == 0 && env_int("MUSICA_HOST_LANES", 1) != 0)) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, host_pixels) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
static bool ensure_lanes(musica_ctx* c) {
    if (!c->lanes.empty()) return true;
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++)
        if (!c->lane_copy[k]) ok = hipStreamCreateWithFlags(&c->lane_copy[k], hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < kLaneStreams && ok; k++) {
        if (!c->lane_stream[k]) ok = ok && hipStreamCreateWithFlags(&c->lane_stream[k], hipStreamNonBlocking) == hipSuccess;
        if (!c->lane_done[k]) ok = ok && hipEventCreateWithFlags(&c->lane_done[k], hipEventDisableTiming) == hipSuccess;
    }
    if (ok && !c->lane_start) ok = hipEventCreateWithFlags(&c->lane_start, hipEventDisableTiming) == hipSuccess;
    while (ok && (int)c->img_copied.size() < c->B) {
        hipEvent_t e = nullptr;
        ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (ok) c->img_copied.push_back(e);
    }
    if (!ok) return false;
    // images per lane: the chain of a lane should be shorter than its copy, or the lanes queue up behind each other instead of behind the
    // link — one 2048^2 image: 0.17 - 0.19 ms of kernels against 0.155 ms of copy; two: 0.18 ms against 0.31 ms
    const int per = c->B >= 4 ? 2 : 1;
    for (int k = 0; k < c->B; k += per) {   // last: c->lanes non-empty means everything above exists
        musica_ctx* v = make_lane(c, k, c->B - k < per ? c->B - k : per);
        v->stream = c->lane_stream[(k / per) % kLaneStreams];
        v->cur = v->stream;
        c->lanes.push_back(v);
    }
    return true;
}
// One batch from host memory into `d_dst` (c->d_input or the streaming path's second buffer), image by image: copy k on the copy
// stream, image k's one-stream script behind it on lane stream k % 3; the context's own stream continues when every lane has finished.
// `after`: an event the copies must wait for (the buffer's previous reader), or null.
static int enqueue_images_from_host(musica_ctx* c, uint16_t* d_dst, const uint16_t* pixels, bool copies_wait = true) {
    const size_t NN = (size_t)c->N * c->N;
    reset_tickets_if_needed(c);
    // whatever the context's stream still runs (the previous step: it reads and writes the planes the lanes are about to overwrite) comes
    // first; the copies too unless the caller knows `d_dst` is free (the streaming path's double buffer)
    hipEventRecord(c->lane_start, c->stream);
    if (copies_wait) { hipStreamWaitEvent(c->lane_copy[0], c->lane_start, 0); hipStreamWaitEvent(c->lane_copy[1], c->lane_start, 0); }
    for (int k = 0; k < kLaneStreams; k++) hipStreamWaitEvent(c->lane_stream[k], c->lane_start, 0);
    // every copy first (the host takes ~100 us to enqueue one lane's replay: with copy k + 1 enqueued behind lane k the copy engine
    // idled between the images — 1.68 ms for the eight copies of 8 x 2048^2 instead of 1.24), then the lanes
    int first = 0;
    for (size_t l = 0; l < c->lanes.size(); l++) {
        const int nb = c->lanes[l]->B;
        if (hipMemcpyAsync(d_dst + (size_t)first * NN, pixels + (size_t)first * NN, (size_t)nb * NN * sizeof(uint16_t), hipMemcpyHostToDevice, c->lane_copy[0]) != hipSuccess)
            return fail("host-to-device copy of images %d.. failed: %s", first, hipGetErrorString(hipGetLastError()));
        hipEventRecord(c->img_copied[l], c->lane_copy[0]);
        first += nb;
    }
    first = 0;
    int ok = 1;
    for (size_t l = 0; l < c->lanes.size() && ok; l++) {
        musica_ctx* v = c->lanes[l];
        const int k = first;
        first += v->B;
        hipStreamWaitEvent(v->stream, c->img_copied[l], 0);
        v->cur_input = d_dst + (size_t)k * NN;
        v->cur = v->stream;
        ok = enqueue_all_impl(v);
    }
    // also after a failed lane: what the lanes before it enqueued still writes the planes, and musica_sync waits on c->stream only
    for (int k = 0; k < kLaneStreams; k++) {
        hipEventRecord(c->lane_done[k], c->lane_stream[k]);
        hipStreamWaitEvent(c->stream, c->lane_done[k], 0);
    }
    if (!ok) { c->needs_reset = true; return 0; }
    c->cur_input = d_dst;
    step_done(c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->needs_reset = true; return fail("per-image dispatch failed: %s", hipGetErrorString(e)); }
    return 1;
}

int musica_sync(musica_ctx* c) {
    CHECK_CTX(c);
    {
        const hipError_t e_ = hipStreamSynchronize(c->stream);
        if (e_ != hipSuccess) { c->needs_reset = true; return fail("hipStreamSynchronize failed: %s", hipGetErrorString(e_)); }
    }
    if (c->profiling) collect_spans(c);
    return 1;
}

int musica_upload(musica_ctx* c, const uint16_t* pixels) {
    CHECK_CTX(c);
    if (!pixels) return fail("musica_upload: pixels is NULL");
    HIP_OK(hipMemcpyAsync(c->d_input, pixels, (size_t)c->B * c->N * c->N * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 1;
}

int musica_execute_device(musica_ctx* c, const uint16_t* d_pixels) {
    CHECK_CTX(c);
    if (!d_pixels) return fail("musica_execute_device: d_pixels is NULL");
    if (((uintptr_t)d_pixels & 15u) != 0) return fail("musica_execute_device: d_pixels must be 16-byte aligned");
    c->cur_input = d_pixels;
    if (!enqueue_all(c)) return 0;
    c->stepped = true;
    return 1;
}

int musica_execute(musica_ctx* c, const uint16_t* pixels) {
    ABI_TRY
    CHECK_CTX(c);
    if (!pixels) return fail("musica_execute: pixels is NULL");
    if (lanes_wanted(c, pixels)) {   // a batch in pinned memory: image k's chain starts when image k has landed (the copy of a batch takes 2 - 3 x its kernels)
        if (!ensure_lanes(c)) return fail("musica_execute: stream / event creation for the image lanes failed");
        if (!enqueue_images_from_host(c, c->d_input, pixels, true)) return 0;
        c->stepped = true;
        return musica_sync(c);
    }
    HIP_OK(hipMemcpyAsync(c->d_input, pixels, (size_t)c->B * c->N * c->N * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));  // vk_state.cpp:313-342
    c->cur_input = c->d_input;
    if (!enqueue_all(c)) return 0;
    c->stepped = true;
    return musica_sync(c);  // vkWaitForFences, src/vk_processing.cpp:2535-2536
    ABI_CATCH("musica_execute")
}

// The reference uploads every image through a freshly allocated staging buffer and three queue-idle waits before a single
// dispatch starts (VulkanState::loadDataToImage, src/vk_state.cpp:313-342). A sequence of batches is pipelined instead: two
// device input buffers, host-to-device copies on a stream of their own, so the copy of batch j + 1 runs under the kernels of
// batch j and the host only blocks at the very end. Input in pinned memory (musica_host_alloc) moves at the PCIe rate;
// pageable memory works too (the runtime stages it, slower and partly synchronous).
int musica_execute_stream(musica_ctx* c, const uint16_t* const* pixels, uint32_t count, musica_stats* stats) {
    ABI_TRY
    CHECK_CTX(c);
    if (!pixels) return fail("musica_execute_stream: pixels is NULL");
    const size_t bytes = (size_t)c->B * c->N * c->N * sizeof(uint16_t);
    if (!c->ev_consumed[1]) {   // keyed on the LAST resource of the block: a call that failed half-way is retried, never half-initialised
        if (!ensure(c, &c->d_input2, (size_t)c->B * c->N * c->N)) return fail("musica_execute_stream: device allocation failed");
        if (!c->copy_stream) HIP_OK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) {
            if (!c->ev_copied[k]) HIP_OK(hipEventCreateWithFlags(&c->ev_copied[k], hipEventDisableTiming));
            if (!c->ev_consumed[k]) HIP_OK(hipEventCreateWithFlags(&c->ev_consumed[k], hipEventDisableTiming));
        }
    }
    if (count == 0) return 1;
    // (Whole batches: the copy of batch j + 1 under the kernels of batch j already moves the pixels at the rate the link delivers — 53 - 54 GB/s
    // here. The image lanes of musica_execute were measured in this loop too: 20 - 22 GP/s against 26.5, the host needs ~0.8 ms per batch
    // to enqueue eight replays and the next batch's copies wait behind that.)
    musica_stats* d_rows = nullptr;
    musica_stats* h_rows = nullptr;
    struct RowsGuard {   // the two scratch buffers go away on every exit path
        musica_stats*& d; musica_stats*& h;
        ~RowsGuard() { if (d) hipFree(d); if (h) hipHostFree(h); }
    } rows_guard{d_rows, h_rows};
    if (stats) {
        HIP_OK(hipMalloc(&d_rows, (size_t)count * c->B * sizeof(musica_stats)));
        if (hipHostMalloc(&h_rows, (size_t)count * c->B * sizeof(musica_stats), hipHostMallocDefault) != hipSuccess) { h_rows = nullptr; return fail("musica_execute_stream: pinned allocation failed"); }
    }
    HIP_OK(hipStreamSynchronize(c->stream));   // nothing of an earlier call still reads the input buffers
    uint16_t* bufs[2] = {c->d_input, c->d_input2};
    int ok = 1;
    for (uint32_t j = 0; j < count && ok; j++) {
        const int k = (int)(j & 1u);
        if (!pixels[j]) { ok = fail("musica_execute_stream: pixels[%u] is NULL", j); break; }
        // batch j - 2 has been computed: its buffer is free. Waited for on the HOST: a copy-engine queue that waits for a compute
        // queue's event stalls for ~1 ms at a time on this part (one 2048^2 image per batch: 1.3 ms per batch with the wait on the copy
        // stream against 0.2 here; devtools/stream_probe.py), and the host has nothing else to do before it may enqueue this copy
        if (j >= 2 && hipEventSynchronize(c->ev_consumed[k]) != hipSuccess) { ok = fail("musica_execute_stream: waiting for batch %u failed", j - 2); break; }
        if (hipMemcpyAsync(bufs[k], pixels[j], bytes, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess) { ok = fail("musica_execute_stream: H2D copy failed"); break; }
        hipEventRecord(c->ev_copied[k], c->copy_stream);
        hipStreamWaitEvent(c->stream, c->ev_copied[k], 0);
        c->cur_input = bufs[k];
        ok = enqueue_all(c);
        if (ok) c->stepped = true;
        if (ok && stats) {
            launch_stats(c->stream, c->d_cnr, c->lv[MUSICA_CNR_LEVEL], c->d_minmax, c->min_chain_exact, c->d_noise_max, c->L, c->d_grad_max, c->d_gcurve,
                         d_rows + (size_t)j * c->B, j * (uint32_t)c->B, 1u, c->B, c->d_stats_partial);
        }
        hipEventRecord(c->ev_consumed[k], c->stream);
    }
    if (ok && stats) ok = hipMemcpyAsync(h_rows, d_rows, (size_t)count * c->B * sizeof(musica_stats), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    const hipError_t e = hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->copy_stream);
    if (ok && e == hipSuccess && stats) memcpy(stats, h_rows, (size_t)count * c->B * sizeof(musica_stats));
    if (e != hipSuccess) return fail("musica_execute_stream: %s", hipGetErrorString(e));
    if (c->profiling) collect_spans(c);
    return ok;
    ABI_CATCH("musica_execute_stream")
}

int musica_debug_run_stage(musica_ctx* c, musica_stage stage) {
    CHECK_CTX(c);
    c->cur = c->stream;
    const StepForm f = step_form(c, STEP_STAGE);   // one launch per level and stage, whatever the context's whole steps run
    switch (stage) {
        case MUSICA_STAGE_NORM: enqueue_norm(c, false); break;
        case MUSICA_STAGE_REDUCE: enqueue_reduce(c, f, 0, c->L); break;
        case MUSICA_STAGE_ANALYSIS:
            launch_clear(c->stream, nullptr, c->d_noise_hist, nullptr, nullptr, c->B);
            enqueue_sdev_from(c, f, 0);
            run_curves_cnr(c);
            c->sdev_stored = true;   // the single-stage form stores every level's sdev image
            break;
        case MUSICA_STAGE_EXPAND: ensure_sdev(c); enqueue_expand(c, f, c->L - 1, 0, false); break;
        case MUSICA_STAGE_GRADATION:
            launch_clear(c->stream, nullptr, nullptr, c->d_grad_hist, c->d_clahe_hist, c->B, c->d_grad_hist_b, c->d_gzero);
            enqueue_gradation(c, false);
            break;
        default: return fail("musica_debug_run_stage: unknown stage %d", (int)stage);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(e));
    return musica_sync(c);
}

}  // extern "C"
