// ugsm_policy.cpp -- which kernel and which stream a level gets, and nothing that enqueues.
//
// Which kernel runs a level is decided by the level's size -- compared with what the LAUNCH holds: pairs x W x H, pairs = the batch where
// the level is batched, else 1 -- and by ONE question: does the call have the chip to itself (Slot::alone; call_alone below)?  A call alone
// wants every launch SHORT: nothing else fills the CUs a launch leaves idle.  A call that shares the chip wants every launch to do LITTLE
// REDUNDANT WORK: what it wastes, the others could have used.  Five choices ask the question (marked ALONE below, plus the pyramid's
// streaming threshold and the side stream); the rest is six numbers.  The A/B behind each: DESIGN.md section 4.
// (Rounds 3-5 switched between two whole threshold sets by ugsm_config.slots and the frame size; forced against each other they differ by
// 0.35 % where bench.py measures, and a lone 16 MP call on a four-slot context lost 11.6 % to the wrong one: VERDICT r05 #1.)
// Below: the six numbers and the choices that follow from a level's size; the choices that ask what else is in flight (level 0 from the image,
// the pyramid's streaming kernel, the side stream, call_alone); what makes a batch run pair by pair; the development overrides; and
// ugsm_plan_level, which reports all of it without a device.
#include "ugsm_device.hpp"
#include "ugsm_slot.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace ugsm;

namespace ugsm {

constexpr long long kBatchMaxPixels = 9000000;  // levels up to here go through a batched call as ONE launch for all its pairs (level 0 of a 16 MP pair: pair by pair)
constexpr int kSmallMaxPixelsAlone = 150000;    // the coarse levels' latency kernels (ugsm_kernels_small.hip) up to here for a call alone ...
constexpr int kSmallMaxPixelsShared = 50000;    // ... and up to here on a shared chip (above it k_cost_march4 and the tiled K-smooth redo less)
constexpr int kMarch4MaxPixels = 3000000;       // above them k_cost_march4 (four waves per strip: wins while a launch lasts as long as one strip) up to here
constexpr int kMarchMinPixels = 400000;         // k_cost_march from here -- asked after k_cost_march4, so in effect above its range
constexpr int kSmoothBigMinPixels = 1 << 19;    // k_smooth_fused's 112-column tile from here (1.39 x the tile in halo work, against 1.8 x for 64 x 32)

bool batch_level(const ugsm_ctx *ctx, int W, int H)
{
    const long long thr = ctx->batch_max_px > 0 ? ctx->batch_max_px : (ctx->batch_max_px < 0 ? 0 : kBatchMaxPixels);
    return (long long)W * H <= thr;
}

// entries per launch of a batched level of a call of nb entries: all of them; the 2 x 9 .. 2 x 16 entries of a checked foveated call
// in launches of equal size, none above kMaxBatch (what a Batch holds)
int group_pairs(int nb)
{
    const int launches = (nb + kMaxBatch - 1) / kMaxBatch;
    return (nb + launches - 1) / launches;
}
// entries a launch of a W x H level of a call of this shape holds
int launch_pairs(const ugsm_ctx *ctx, const Shape &sh, int W, int H) { return (sh.nb > 1 && batch_level(ctx, W, H)) ? group_pairs(sh.nb) : 1; }

static int small_max_px(const ugsm_config &cfg, bool alone)
{
    if (cfg.small_max_pixels < 0) return 0;
    return cfg.small_max_pixels > 0 ? cfg.small_max_pixels : (alone ? kSmallMaxPixelsAlone : kSmallMaxPixelsShared);
}
bool use_march4(const ugsm_ctx *ctx, int W, int H, bool alone, int pairs)
{
    const long long px = (long long)W * H * pairs;
    if (ctx->cfg.kernel_path == 1) return false;
    if (ctx->march4_hi >= 0) return ctx->march4_hi > 0 && px >= ctx->march4_lo && px <= ctx->march4_hi;  // (development override)
    return px > small_max_px(ctx->cfg, alone) && px <= kMarch4MaxPixels;
}
static bool march_by_size(const ugsm_ctx *ctx, int W, int H, int pairs)  // (ugsm_config.march_min_pixels moves the threshold: tests run every level through it)
{
    const int thr = ctx->cfg.march_min_pixels;
    return thr >= 0 && (long long)W * H * pairs >= (thr > 0 ? thr : kMarchMinPixels);
}
int march_rows_arg(const ugsm_ctx *ctx) { return ctx->cfg.march_rows > 0 ? ctx->cfg.march_rows : ctx->march_mode; }

// The latency kernels' K-smooth region height (0 = not a level of theirs).  On a shared chip 18 x 18 tiles (3.2 x the tile in halo work; the
// 18 x 4 / 18 x 10 tiles redo 8 x / 4.6 x: free on an idle chip, 3.6 % / 9.2 % of the throughput with four pairs in flight); a call ALONE
// takes the smallest tile that still gives every workgroup a CU of its own, or nearly.
int small_rh(const ugsm_ctx *ctx, int W, int H, bool alone, int pairs)
{
    const long long px = (long long)W * H * pairs;
    if (ctx->cfg.small_max_pixels < 0 || ctx->cfg.kernel_path == 1 || px > small_max_px(ctx->cfg, alone) || march_by_size(ctx, W, H, pairs)) return 0;
    if (ctx->small_rh_force) return ctx->small_rh_force;
    return !alone ? 32 : (px <= 36000 ? 18 : (px <= 80000 ? 24 : 32));
}
bool use_small_cost(const ugsm_ctx *ctx, int W, int H, bool alone, int pairs)
{
    return (ctx->small_mask & 1) && small_rh(ctx, W, H, alone, pairs) != 0;
}
// k_cost_march: the levels of at least march_min_pixels per launch, and every level that no other form covers -- it is the one shipped form
// with no size limit and a batch index.  With the default thresholds the other forms cover every size below kMarch4MaxPixels by
// themselves; the fallback takes what a configuration leaves uncovered (march_min_pixels above k_cost_march4's reach, small_max_pixels < 0
// with k_cost_march4 off, the development switches).  Only march_min_pixels < 0 (libugsm_dev.so) leaves such levels to round 1's
// LDS-tiled k_cost_split.
bool use_march(const ugsm_ctx *ctx, int W, int H, bool alone, int pairs)
{
    if (ctx->cfg.kernel_path == 1 || ctx->cfg.march_min_pixels < 0) return false;
    return march_by_size(ctx, W, H, pairs) || (!use_march4(ctx, W, H, alone, pairs) && !use_small_cost(ctx, W, H, alone, pairs));
}

// Seeding (subsampleDisp, MatchGPULib.cpp:1526-1590) rides on the level's first K-cost launch when that is a marching kernel: the seeded field is
// never written.  Not with the early exit (the field before the first iteration is compared against), not on the one-stage-per-kernel path.
bool fuse_seed(const ugsm_ctx *ctx, int W, int H, bool alone, int pairs)
{
    return ctx->fuse_seed && ctx->cfg.kernel_path != 1 && !(ctx->cfg.early_exit_threshold > 0.0f) && (use_march(ctx, W, H, alone, pairs) || use_march4(ctx, W, H, alone, pairs));
}

// k_smooth_fused's tile: > 0 = the 112-column tile at this height -- a call ALONE picks the height that fills whole rounds of workgroups
// (smooth_tile_rows), else 36 --; 0 = the tile class by the level's size (64 x 32 from 0.26 Mpx, else 32 x 16)
int smooth_rows_for(const ugsm_ctx *ctx, int W, int H, bool alone, int pairs)
{
    if ((long long)W * H * pairs < (ctx->smooth_big_min > 0 ? ctx->smooth_big_min : kSmoothBigMinPixels)) return 0;
    if (pairs > 1 && W < 100) return 0;  // (a level narrower than the 112-column tile: the smaller tile classes waste fewer lanes)
    if (ctx->smooth_rows > 0) return std::min(ctx->smooth_rows, kSmoothTileRowsMax);
    return smooth_tile_rows(W, H, ctx->smooth_rows == -1 ? 1 : (ctx->smooth_rows == -2 ? 0 : (alone ? 1 : 0)), pairs);
}
// ... and the tile class of the smaller levels of a batched launch: by what the launch holds
int smooth_class_for(int W, int H, int pairs)
{
    return pairs <= 1 ? 0 : (((long long)W * H * pairs >= smooth_mid_min_pixels && W >= 48 && H >= 24) ? 2 : 1);
}

// Level 0 of the pyramid is (float) of each byte of the image: it holds nothing the image does not, and at 16 MP storing it is 193 of the 338 MB
// the pyramid pass writes per image.  A full-mode call therefore leaves it unwritten and its level-0 launches -- A = G_clamp * L^2 and K-cost,
// which run last -- read the image itself: the caller's device buffer, which stays valid and untouched until the call is reported
// (include/ugsm.h), or the slot's own upload.  Where: the fused path's k_pyr_base (three levels or more), level 0 matched by k_cost_march (the
// one K-cost form with an 8-bit instance: the levels that large), rgb8 images (the other layouts keep the float level 0: eight more K-cost
// bodies per layout for formats no measured workload uses), no early exit (it runs pair by pair through other buffers).  Everything
// that hands the pyramids on -- ugsm_submit_pyramids, the foveated calls, the stage entry points -- stores level 0 as ever.
// entries: how many fields the call runs in lockstep (0: the slot's pairs; a checked full-mode call: two per pair) -- what a launch holds decides the kernel.
bool level0_direct(const ugsm_ctx *ctx, const Slot &s, int entries)
{
    if (ctx->level0_float || ctx->cfg.kernel_path == 1 || ctx->cfg.early_exit_threshold > 0.0f || s.levels < 3) return false;
    if (ctx->hooks.input_format != kInRGB8) return false;
    Shape sh = Shape::pairs(s);
    if (entries > 0) sh.nb = entries;
    const int pairs = launch_pairs(ctx, sh, s.W, s.H);
    return !use_march4(ctx, s.W, s.H, s.alone, pairs) && use_march(ctx, s.W, s.H, s.alone, pairs);
}

// One full-mode pair alone on the chip: the streaming factor-2 kernel's many short workgroups on the side stream get
// in the way of the main stream's latency-bound launches -- 112.3 pairs/s with it on every level, 114.4 with it on the launches of
// >= 1.5 M outputs only, 114.1 without it (tools/ab.py, same box); foveated calls and everything with more in flight gain from it
// on every level (a lone foveated pair +1.8 %, batches of eight +3.3 %).
// windowed: the call is foveated (its pyramid kernels store level 0 inside the windows only).
long long pyramid_stream_min(const Slot &s, bool windowed) { return (s.alone && s.nb == 1 && !windowed) ? 1500000 : 0; }

// Whether this call may use the slot's side stream: single pairs that have the chip to themselves (with four pairs in flight eight
// streams on the four hardware queues serialise what one stream per pair lets overlap: -13 %), the fused path, no event brackets (the
// statistics belong to one stream).
bool side_stream_ok(const ugsm_ctx *ctx, const Slot &s)
{
    return s.nb == 1 && s.alone && s.st2 != nullptr && ctx->cfg.kernel_path != 1 && ctx->cfg.profile_events == 0 && ctx->two_streams;
}

// Has everything enqueued on the slot finished?  (Never blocks; a slot found idle stops counting as busy.)
static bool slot_idle(Slot &s)
{
    if (!s.busy) return true;
    const hipError_t e = s.done_recorded ? hipEventQuery(s.ev_done) : hipStreamQuery(s.st);
    if (e == hipErrorNotReady) return false;
    if (e != hipSuccess) (void)hipGetLastError();  // (the slot's own ugsm_wait / ugsm_poll reports it)
    s.busy = false;
    return true;
}
// Does the call about to be enqueued on `slot` have the chip to itself?  It does when nothing is unfinished on any other slot of the
// context and the dispatcher has not said that more calls follow (the queue, ugsm_queue.cpp: pairs wait behind this call, or a call
// filled up by itself -- a host that submits faster than the chip matches).  The blocking entry points (ugsm_match_*: the node's service
// call, UG_GPU_matcher.cpp:497-694, and its one-at-a-time topic path, :126-185) are therefore alone whatever ugsm_config.slots says; a
// burst through the slot API is alone for its first call only.  What is in flight decides -- not how many slots the context was created
// with.
bool call_alone(ugsm_ctx *ctx, int slot)
{
    if (ctx->force_alone >= 0) return ctx->force_alone == 1;
    if (ctx->hooks.queue_calling && ctx->hooks.queue_more) return false;
    for (int i = 0; i < (int)ctx->slots.size(); i++)
        if (i != slot && !slot_idle(ctx->slots[i])) return false;
    return true;
}

// The LR check's setting (ugsm_set_lr_check): which calls apply it
bool lr_full_on(const ugsm_ctx *ctx) { return ctx->lr_tau > 0.0f && (ctx->lr_modes & UGSM_LR_FULL); }
bool lr_fovea_on(const ugsm_ctx *ctx) { return ctx->lr_tau > 0.0f && (ctx->lr_modes & UGSM_LR_FOVEATED); }
// Contexts whose options need a host round trip per iteration, a second match, or the one-kernel-per-stage path run their batches pair by pair.
bool batch_runs_pair_by_pair(const ugsm_ctx *ctx) { return ctx->cfg.kernel_path == 1 || ctx->cfg.early_exit_threshold > 0.0f || lr_full_on(ctx); }
// ... and the foveated batches: the foveated check runs in lockstep (enqueue_foveated; ugsm_set_lr_check refuses it to the contexts of the
// first two kinds).  A context with the full-mode check alone sends its foveated batches through pair by pair as it always has.
bool fovea_batch_runs_pair_by_pair(const ugsm_ctx *ctx) { return batch_runs_pair_by_pair(ctx) && !lr_fovea_on(ctx); }
// ... and the n windows of one pair (ugsm_submit_foveated_multi): their fine phase runs window after window, as single pairs, in the contexts of the
// first two kinds; a lone window is a single pair.  (The checked form is refused to those contexts and runs a lone window in lockstep with its twin.)
bool fovea_windows_run_one_by_one(const ugsm_ctx *ctx, int n) { return n == 1 || ctx->cfg.kernel_path == 1 || ctx->cfg.early_exit_threshold > 0.0f; }

// ---- development overrides ---------------------------------------------------------------
// tools/ and tests/ steer the per-level kernel choice through environment variables.  They are read ONLY when UGSM_DEV=1 is set
// as well, so that a production process never changes behaviour because of a stray variable, and in ONE place, shared by
// ugsm_create and ugsm_plan_level (which therefore reports what a context created under the same environment launches).
// (DevKnobs: ugsm_slot.hpp.)
static bool dev_env_on()
{
    const char *e = getenv("UGSM_DEV");
    return e && e[0] == '1';
}
bool dev_env() { return dev_env_on(); }
// set_globals: also apply the process-wide tuning variables (UGSM_SMOOTH_MID_MIN, UGSM_PYR_STREAM*, UGSM_MARCH_AGE).  They are CREATE-TIME,
// PROCESS-WIDE settings: ugsm_create applies them only while no other context of the process is alive (g_live_contexts, under
// g_globals_mutex: ugsm_runtime.cpp), so that creating a second context never changes the kernels of a live one, from whatever thread; the
// host-only ugsm_plan_level never does.
void apply_dev_env(ugsm_config &cfg, DevKnobs &k, bool set_globals)
{
    if (!dev_env_on()) return;
    auto geti = [](const char *name, int &dst) {
        if (const char *e = getenv(name)) dst = atoi(e);
    };
    geti("UGSM_KERNEL_PATH", cfg.kernel_path);
    geti("UGSM_MARCH_MIN_PIXELS", cfg.march_min_pixels);
    geti("UGSM_MARCH_ROWS", cfg.march_rows);
    geti("UGSM_SMALL_MAX_PIXELS", cfg.small_max_pixels);
    geti("UGSM_SMALL_MASK", k.small_mask);
    geti("UGSM_FUSE_SEED", k.fuse_seed);
    geti("UGSM_TWO_STREAMS", k.two_streams);
    geti("UGSM_SMOOTH_ROWS", k.smooth_rows);
    geti("UGSM_MARCH_MODE", k.march_mode);
    geti("UGSM_LEVEL0_FLOAT", k.level0_float);
    if (const char *e = getenv("UGSM_STREAM_PRIO")) snprintf(k.stream_prio, sizeof k.stream_prio, "%s", e);
    if (const char *e = getenv("UGSM_SIDE_PRIO")) k.side_prio = e[0];
    if (const char *e = getenv("UGSM_ALONE")) k.force_alone = e[0] == '1' ? 1 : (e[0] == '0' ? 0 : -1);
    geti("UGSM_SMOOTH_BIG_MIN", k.smooth_big_min);
    if (const char *e = getenv("UGSM_BATCH_MAX_PIXELS")) k.batch_max_px = atoll(e);
    if (set_globals) {  // the process-wide tuning variables: back to their defaults first, so that a variable a test has removed stops acting
        smooth_mid_min_pixels = 1 << 18;
        smooth_lds_extra_bytes = 0;
        blur_decimate_streaming = 1;
        pyr_base_streaming = 1;
        blur_decimate_streaming_min = 0;
        march_age_permille[0] = 470;
        march_age_permille[1] = 340;
        geti("UGSM_SMOOTH_MID_MIN", smooth_mid_min_pixels);
        geti("UGSM_SMOOTH_LDS_EXTRA", smooth_lds_extra_bytes);
        geti("UGSM_PYR_STREAM", blur_decimate_streaming);
        geti("UGSM_PYR_BASE_STREAM", pyr_base_streaming);
        if (const char *e = getenv("UGSM_PYR_STREAM_MIN")) blur_decimate_streaming_min = atoll(e);
    }
    if (const char *e = set_globals ? getenv("UGSM_MARCH_AGE") : nullptr) {
        int a = 0, b = 0;
        if (sscanf(e, "%d,%d", &a, &b) == 2 && a >= 0 && b >= 0 && a + b < 1000) {
            march_age_permille[0] = a;
            march_age_permille[1] = b;
        }
    }
    if (const char *e = getenv("UGSM_MARCH4")) {
        int a = 0, b = 0;
        if (sscanf(e, "%d,%d", &a, &b) == 2 && a >= 0 && b >= a) {
            k.march4_lo = a;
            k.march4_hi = b;
        }
    }
    int rh = 0;
    geti("UGSM_SMALL_RH", rh);
    if (rh == 18 || rh == 24 || rh == 32) k.small_rh_force = rh;
}

// The choices of a context that are not in ugsm_config: the development overrides (the defaults are with the policy functions below).
void set_policy(ugsm_ctx *c, const DevKnobs &k)
{
    c->small_mask = k.small_mask;
    c->fuse_seed = k.fuse_seed;
    c->small_rh_force = k.small_rh_force;
    c->smooth_rows = k.smooth_rows;
    c->smooth_big_min = k.smooth_big_min > 0 ? k.smooth_big_min : 0;
    // strips by age class, every context: +8 % on a level-0 launch alone on the chip, +1.2 % on a pair alone; with four pairs in
    // flight it costs 0.4 % (163.2 against 163.7 pairs/s) -- kept on there too, so that a kernel measured alone is the kernel that ran
    c->march_mode = k.march_mode <= 0 ? k.march_mode : 0;
    c->march4_lo = k.march4_lo;
    c->march4_hi = k.march4_hi;
    c->force_alone = k.force_alone;
    c->batch_max_px = k.batch_max_px;
    c->level0_float = k.level0_float;
}

}  // namespace ugsm

extern "C" {

int ugsm_plan_level(const ugsm_config *cfg_in, int alone, int W, int H, ugsm_level_plan *out)
{
    if (!out || W < 1 || H < 1) return UGSM_ERR_BAD_ARG;
    ugsm_ctx probe;  // host-only: the same policy functions the launch path calls, on a context that owns no device state
    if (cfg_in) probe.cfg = *cfg_in;
    else ugsm_default_config(&probe.cfg);
    {   // ... under the same development overrides ugsm_create would apply in this process (none unless UGSM_DEV=1)
        DevKnobs knobs;
        apply_dev_env(probe.cfg, knobs, false);
        set_policy(&probe, knobs);
    }
    UCHK(check_config(probe.cfg));  // (what ugsm_create refuses has no plan)
    memset(out, 0, sizeof *out);
    if (probe.cfg.kernel_path == 1) {
        out->cost_kernel = out->smooth_kernel = 3;
        out->pairs_per_launch = 1;
        return UGSM_OK;
    }
    // a context created for batches (ugsm_config.batch) is asked about a call of that many pairs: a level of at most kBatchMaxPixels is one
    // launch for all of them, and the thresholds are compared with what the launch holds
    const int nb = std::min(std::max(probe.cfg.batch, 1), kMaxBatch);
    const bool al = probe.force_alone >= 0 ? probe.force_alone == 1 : alone != 0;
    out->alone = al ? 1 : 0;
    const int pairs = (nb > 1 && batch_level(&probe, W, H)) ? nb : 1;
    const bool march4 = use_march4(&probe, W, H, al, pairs);  // (asked first, as in run_level)
    const bool march = use_march(&probe, W, H, al, pairs);
    const int rh = small_rh(&probe, W, H, al, pairs);
    out->cost_kernel = march4 ? 4 : (march ? 1 : (use_small_cost(&probe, W, H, al, pairs) ? 2 : 0));
    out->smooth_kernel = (rh && (probe.small_mask & 2)) ? 2 : 0;
    out->smooth_rh = (probe.small_mask & 2) ? rh : 0;
    out->strip_rows = march4 ? march4_strip_rows(W, H, pairs)
                             : (march ? (probe.cfg.march_rows > 0 ? probe.cfg.march_rows : march_strip_rows(W, H, probe.march_mode <= -2, pairs)) : 0);
    out->seed_fused = fuse_seed(&probe, W, H, al, pairs) ? 1 : 0;
    out->smooth_tile_rows = out->smooth_kernel == 0 ? smooth_rows_for(&probe, W, H, al, pairs) : 0;
    out->pairs_per_launch = pairs;
    return UGSM_OK;
}

}  // extern "C"
