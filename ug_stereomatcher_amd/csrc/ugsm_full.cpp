// ugsm_full.cpp -- the full-frame descent (enqueue_descent: the loop of matching(), coarse to fine) and the calls that are made of it: the
// whole call, its LR check the old way (a second descent) and the new (both directions in lockstep), the seeded call, the two halves -- and the
// coarse phase of a foveated call, which is the same descent stopped at level F-1 (the rest of a foveated call: ugsm_fovea.cpp).  The levels'
// own work is ugsm_levels.cpp.  At the end the ugsm_submit_* entry points of the family.
#include "ugsm_device.hpp"
#include "ugsm_slot.hpp"

#include <algorithm>

using namespace ugsm;

namespace ugsm {
namespace {

// the full-frame views of level `lev` for every entry of the call (a shape of real pairs)
void full_views(const Slot &s, const Shape &sh, const float *pyr, int lev, Img3 *out)
{
    for (int b = 0; b < sh.nb; b++) out[b] = level_view(s, pyr + b * s.pyr_stride, lev, 0, 0);
}

void side_views(const Slot &s, const Shape &sh, int side, int lev, Img3 *out)
{
    for (int v = 0; v < sh.nb; v++) out[v] = level_view(s, pair_pyr(s, sh, side, v), lev, 0, 0);
}

// A of full-frame level i if it was precomputed on the side stream (the main stream is made to wait for it here), else null
const float *level_A(ugsm_ctx *ctx, Slot &s, int i)
{
    if (s.a_from < 0 || i < s.a_from) return nullptr;
    if (hipStreamWaitEvent(s.st, s.ev_A[i], 0) != hipSuccess) return nullptr;
    (void)ctx;
    return s.Apyr + s.off[i];
}

// The full-frame levels from .. to of a call, coarse to fine, for the entries of `sh`: the loop of matching(), MatchGPULib.cpp:1196-1318.
// Which levels, and what level `from` starts from, is the call's LevelRange:
//   Zero (from == top): the zero seed, and level `from` is the top level (its first iteration takes no confidence);
//   Prior: the restriction of the entries' full-resolution fields (launch_restrict) fills level `from`'s fields where the zero seed is
//          otherwise set; the levels above run nothing, and level `from` is no top level, whichever it is -- its first iteration blends the
//          confidence like any other, a prior has one;
//   State: the entries' fields of level from + 1, placed in the level buffer and handed to level `from` by the cold call's own step
//          (hand_seed): the descent goes on at level `from` as if the levels above had just run.
// From there down everything is the same.  What else differs between the callers comes in:
// views(i, Lv, Rv): fills the entries' views of level i and returns their form (run_level's `in`);
// side_A: a level's A is taken from the side stream where it was precomputed there (level_A);
// direct_out (optional): the entries' result buffers, which level 0's last smoothing launch writes itself where it can (no 193 MB device
// copy at 16 MP): `field` is then null.  Otherwise `field` is the level buffer that holds level `to`'s fields, for the caller's copy.
template <class Views>
int enqueue_descent(ugsm_ctx *ctx, Slot &s, int si, const Shape &sh, const LevelRange &r, Views &&views, bool side_A, float *const *direct_out, float *&field)
{
    float *cur = s.d0, *other = s.d1;
    const int from = r.from;
    SeedMap sm[2 * kMaxBatch];  // (a shape of both directions: two entries per pair)
    bool seeded = false;
    if (r.start == LevelRange::State) {
        s.cur_level = from + 1;
        for (int b = 0; b < sh.nb; b++)
            HIPCHK(ctx, hipMemcpyAsync(cur + b * sh.stride, r.source[b], sizeof(float) * 3 * (size_t)s.w[from + 1] * s.h[from + 1], hipMemcpyDeviceToDevice, s.st));
        seeded = hand_seed(ctx, s, si, sh, s.w[from + 1], s.h[from + 1], s.w[from], s.h[from], nullptr, 0, sm, cur, other);
    } else if (r.start == LevelRange::Prior) {
        const float *const *prior = r.source;
        s.cur_level = from;
        for_groups(sh.nb, launch_pairs(ctx, sh, s.w[from], s.h[from]) > 1, [&](Grp g) {
            Timer t(ctx, &s, si, KC_RESTRICT, (double)s.w[from] * s.h[from] * g.n);
            Batch bt{};
            bt.n = g.n;
            for (int j = 0; j < g.n; j++) {
                bt.in[j] = byte_diff(prior[g.b0 + j], prior[g.b0]);
                bt.out[j] = (long long)(j * sh.stride * sizeof(float));
            }
            launch_restrict(s.st, prior[g.b0], s.W, s.H, from, cur + g.b0 * sh.stride, s.w[from], s.h[from], g.n > 1 ? &bt : nullptr);
        });
    } else {
        for (int b = 0; b < sh.nb; b++)  // U1: zero seed
            HIPCHK(ctx, hipMemsetAsync(cur + b * sh.stride, 0, sizeof(float) * 3 * (size_t)s.w[from] * s.h[from], s.st));
    }
    Img3 Lv[2 * kMaxBatch], Rv[2 * kMaxBatch];
    field = nullptr;
    for (int i = from; i >= r.to; i--) {
        s.cur_level = i;
        const int mi = level_iterations(i);
        const bool direct = direct_out && i == 0 && ctx->cfg.kernel_path != 1 && level_smooth(0) > 0 && !(ctx->cfg.early_exit_threshold > 0.0f);
        const int in = views(i, Lv, Rv);
        UCHK(run_level(ctx, s, si, sh, Lv, Rv, s.w[i], s.h[i], mi, level_smooth(i), i == from && r.start == LevelRange::Zero, 1, mi, cur, other, nullptr,
                       direct ? direct_out : nullptr, seeded ? sm : nullptr, side_A ? level_A(ctx, s, i) : nullptr, in));
        if (direct) return UGSM_OK;
        seeded = i > r.to && hand_seed(ctx, s, si, sh, s.w[i], s.h[i], s.w[i - 1], s.h[i - 1], nullptr, 0, sm, cur, other);
    }
    field = cur;
    return UGSM_OK;
}

// the entries' fields of level `lev`, as a descent left them in `field` (entry v at + v * sh.stride), into their destinations
int copy_fields(ugsm_ctx *ctx, Slot &s, const Shape &sh, const float *field, int lev, float *const *outs)
{
    for (int v = 0; v < sh.nb; v++)
        HIPCHK(ctx, hipMemcpyAsync(outs[v], field + v * sh.stride, sizeof(float) * 3 * (size_t)s.w[lev] * s.h[lev], hipMemcpyDeviceToDevice, s.st));
    return UGSM_OK;
}

// matching() with foveatedmatching==0 over the levels of `r`, for the s.nb pairs of the call; d_out: their buffers for level r.to's fields
// (level 0: the results, which its last launch writes itself where it can).
// swap: the images exchanged (the right-to-left match of the LR check): the right pyramid is the "left" image; A is then computed
// in line (the side stream's A planes belong to the left image).
int enqueue_full(ugsm_ctx *ctx, Slot &s, int si, float *const *d_out, const LevelRange &r, bool swap = false)
{
    const Shape sh = Shape::pairs(s);
    const float *const pL = swap ? s.pyrR : s.pyrL, *const pR = swap ? s.pyrL : s.pyrR;
    auto views = [&](int i, Img3 *Lv, Img3 *Rv) -> int {
        if (i == 0 && s.direct0) {  // level 0 was not stored: the images themselves
            for (int b = 0; b < sh.nb; b++) {
                Lv[b] = byte_view(swap ? s.img0R[b] : s.img0L[b], s.img0_stride);
                Rv[b] = byte_view(swap ? s.img0L[b] : s.img0R[b], s.img0_stride);
            }
            return kInRGB8;
        }
        full_views(s, sh, pL, i, Lv);
        full_views(s, sh, pR, i, Rv);
        return kInPlanes;
    };
    float *field;
    UCHK(enqueue_descent(ctx, s, si, sh, r, views, !swap && sh.nb == 1, d_out, field));
    return field ? copy_fields(ctx, s, sh, field, r.to, d_out) : UGSM_OK;
}

// The coarse half's prolongation (ugsm_submit_full_coarse): for the pairs with a d_full entry, the full-resolution field of their level-e
// state in ONE launch (launch_prolong), read from d_state.
int enqueue_prolong(ugsm_ctx *ctx, Slot &s, int si, int e, float *const *d_state, float *const *d_full)
{
    int asked[kMaxBatch], m = 0;
    for (int b = 0; b < s.nb; b++)
        if (d_full[b]) asked[m++] = b;
    if (m == 0) return UGSM_OK;
    Batch bt{};
    bt.n = m;
    for (int j = 0; j < m; j++) {
        bt.in[j] = byte_diff(d_state[asked[j]], d_state[asked[0]]);
        bt.out[j] = byte_diff(d_full[asked[j]], d_full[asked[0]]);
    }
    s.cur_level = e;
    bool launched;
    {
        Timer t(ctx, &s, si, KC_PROLONG, (double)m * s.W * s.H);
        launched = launch_prolong(s.st, d_state[asked[0]], s.w, s.h, e, d_full[asked[0]], m > 1 ? &bt : nullptr);
    }
    if (!launched) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the prolongation: a size its kernel does not cover");
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}


// The context's LR-consistency check of a full-mode call (ugsm_set_lr_check / ugsm_config.lr_check_threshold; no reference counterpart), behind
// the match that wrote d_out: the match with the images exchanged into the slot's own buffer, then one kernel that zeroes the inconsistent
// confidences of d_out.  (Single pairs, whole calls.)
int enqueue_full_lr(ugsm_ctx *ctx, Slot &s, int si, float *d_out)
{
    const float tau = ctx->lr_tau;
    const size_t n3 = 3 * (size_t)s.W * s.H;
    UCHK(lr_ready(ctx, s, n3 + 4));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(s.lr + ((n3 + 1) & ~(size_t)1));  // (8-byte aligned)
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof *cnt, s.st));
    UCHK(enqueue_full(ctx, s, si, &s.lr.p, LevelRange::cold(s.levels), true));
    {
        Timer t(ctx, &s, si, KC_MISC, (double)s.W * s.H);
        launch_lr_check(s.st, d_out, s.lr, s.W, s.H, tau, cnt);
    }
    HIPCHK(ctx, hipMemcpyAsync(s.lr_host, cnt, sizeof *cnt, hipMemcpyDeviceToHost, s.st));
    HIPCHK(ctx, hipGetLastError());
    s.lr_ran = true;
    return UGSM_OK;
}

// The room a checked full-mode call takes in the slot's LR buffer, in floats: one full field (Slot::lvl_stride: a multiple of 64 floats) for
// every pair whose right-to-left field the caller does not take, the count words (one of 8 bytes per (pair, direction)) behind them.
size_t lr_full_room(size_t lvl_stride, int kept, int n) { return (size_t)kept * lvl_stride + 4 * (size_t)n; }

}  // namespace

// ugsm_submit_full_checked: both directions of n full-mode pairs in lockstep, each pair's two fields checked against each other.
//   - the pyramids of the n pairs once, as ugsm_submit_full_batch builds them (a lone pair: the right one on the side stream); level 0 stays
//     unwritten where level0_direct allows, judged by the 2 n entries a launch of the call holds;
//   - one descent over 2 n full-frame entries at a stride of one full field: entry n + b is pair b with the L and R views exchanged (pair_pyr;
//     at level 0 of a direct call: the two images exchanged), under pair b's range word, which covers both of its pyramids.  Every kernel of a
//     level takes the 2 n entries in one launch except K-cost, one launch per direction (cost_groups); more than kMaxBatch entries go through
//     launches of equal size (group_pairs); levels above kBatchMaxPixels run entry by entry.  A is computed in line for both directions;
//   - level 0's last smoothing launch writes the fields where they belong: d_out[b], and d_back[b] or the slot's LR buffer;
//   - one launch of k_lr_check's stack form (F = 1: a stack of one full field) over the 2 n (pair, direction) checks with the call's own tau
//     -- two launches from nine pairs on, an LrStack holds kMaxBatch checks -- and the counts back with one copy.
// The caller has made the level buffers hold 2 n full fields and the LR buffer lr_full_room floats.
int enqueue_full_checked(ugsm_ctx *ctx, Slot &s, int si, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                         float *const *d_out, float *const *d_back, float tau)
{
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, n, W, H, stride, -1, nullptr, true, 2 * n));
    const Shape sh = Shape::full_both_directions(s);
    int kept = 0;
    float *outs[2 * kMaxBatch];
    for (int b = 0; b < n; b++) {
        outs[b] = d_out[b];
        outs[n + b] = (d_back && d_back[b]) ? d_back[b] : s.lr + (size_t)kept++ * s.lvl_stride;
    }
    // (holds already, unless prepare_slot ran out of memory for the configured batch and fell back to this call's n pairs: it then freed what the
    // caller had grown)
    UCHK(ensure_level_bufs(ctx, s, sh.nb * sh.stride));
    if (lr_full_room(s.lvl_stride, kept, n) > s.lr.cap || !s.lr_host) {
        ctx->err = "the slot's buffers do not hold both directions' fields";
        return UGSM_ERR_STATE;
    }
    if (s.range_known) HIPCHK(ctx, hipMemcpyAsync(s.range_bad + n, s.range_bad, sizeof(unsigned) * n, hipMemcpyDeviceToDevice, s.st));
    auto views = [&](int i, Img3 *Lv, Img3 *Rv) -> int {
        if (i == 0 && s.direct0) {  // level 0 was not stored: the images themselves, exchanged for the entries n .. 2 n - 1
            for (int b = 0; b < n; b++) {
                Lv[b] = Rv[n + b] = byte_view(s.img0L[b], s.img0_stride);
                Rv[b] = Lv[n + b] = byte_view(s.img0R[b], s.img0_stride);
            }
            return kInRGB8;
        }
        side_views(s, sh, 0, i, Lv);
        side_views(s, sh, 1, i, Rv);
        return kInPlanes;
    };
    float *field;
    UCHK(enqueue_descent(ctx, s, si, sh, LevelRange::cold(s.levels), views, false, outs, field));
    if (field) UCHK(copy_fields(ctx, s, sh, field, 0, outs));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(s.lr + (size_t)kept * s.lvl_stride);
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof *cnt * 2 * n, s.st));
    // k_lr_check's stack form with F = 1: a "stack" is then one full field.  Check 2 b is pair b's left-to-right field against its right-to-left
    // one, check 2 b + 1 the two exchanged; each reads dx and dy of both fields and writes its own field's confidence alone, so both directions
    // in one launch are race-free and either sees the other's unchecked field.  An LrStack holds kMaxBatch checks: up to eight pairs are one
    // launch, nine to sixteen two of equal size.
    for_groups(2 * n, true, [&](Grp g) {
        LrStack ls{};
        ls.n = g.n;
        ls.F = 1;
        for (int j = 0; j < g.n; j++) {
            const int b = (g.b0 + j) >> 1, dir = (g.b0 + j) & 1;
            ls.fwd[j] = byte_diff(outs[dir ? n + b : b], outs[0]);
            ls.back[j] = byte_diff(outs[dir ? b : n + b], outs[0]);
        }
        Timer t(ctx, &s, si, KC_MISC, (double)g.n * s.W * s.H);
        launch_lr_check(s.st, outs[0], outs[0], s.W, s.H, tau, cnt + g.b0, ls);
    });
    HIPCHK(ctx, hipMemcpyAsync(s.lr_host + 1, cnt, sizeof *cnt * 2 * n, hipMemcpyDeviceToHost, s.st));
    HIPCHK(ctx, hipGetLastError());
    s.lr_ran = true;
    s.lr_full_pairs = n;
    return UGSM_OK;
}

// matching() with foveatedmatching==1 (MatchGPULib.cpp:1230-1294), split at level F-1; d_state: one buffer per entry of the call.
int enqueue_fovea_coarse(ugsm_ctx *ctx, Slot &s, int si, const Shape &sh, float *const *d_state)
{
    const int F = ctx->cfg.fovea_levels;
    if (F < 2 || F > s.levels) return UGSM_ERR_BAD_ARG;
    auto views = [&](int i, Img3 *Lv, Img3 *Rv) -> int {
        side_views(s, sh, 0, i, Lv);
        side_views(s, sh, 1, i, Rv);
        return kInPlanes;
    };
    float *cur;
    UCHK(enqueue_descent(ctx, s, si, sh, LevelRange::coarse(s.levels, F - 1), views, sh.nb == 1, nullptr, cur));
    const size_t fn = (size_t)s.w[F - 1] * s.h[F - 1];
    if (sh.nb == 1) {
        HIPCHK(ctx, hipMemcpyAsync(d_state[0], cur, sizeof(float) * 3 * fn, hipMemcpyDeviceToDevice, s.st));
    } else {
        for_groups(sh.nb, true, [&](Grp g) {
            const Batch bt = copy_batch(sh, g, nullptr, d_state, 0);
            launch_copy_view(s.st, Img3{cur + g.b0 * sh.stride, s.w[F - 1], fn}, s.w[F - 1], s.h[F - 1], d_state[g.b0], fn, s.w[F - 1], &bt);
        });
    }
    return UGSM_OK;
}

// One full-mode call of n pairs on device buffers over the levels of `given` (null: the cold call), every kind of it -- whole, seeded, either half:
//   - the pyramids, as far up as the range reaches: a descent that starts below the top (seeded, fine half) builds the levels 0 .. max(from, 2)
//     only.  A lone pair's A planes come from the side stream, where the call is alone, for the levels the range runs (to .. from); several
//     pairs compute A in line;
//   - the levels of all pairs in lockstep, level `to`'s fields into d_out (level 0: written by its last launch where that can be);
//   - a lone pair's whole call: the context's LR check where it is on (several pairs: no check -- batch_runs_pair_by_pair);
//   - the coarse half: the prolongation of the fields it was asked for.
int enqueue_match_full(ugsm_ctx *ctx, Slot &s, int si, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                             float *const *d_out, const LevelRange *given)
{
    const LevelRange r = given ? *given : LevelRange::cold(ctx->cfg.levels);
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, n, W, H, stride, n == 1 ? r.to : -1, nullptr, true, 0, r.start == LevelRange::Zero ? -1 : r.from));
    UCHK(enqueue_full(ctx, s, si, d_out, r));
    if (n == 1 && r.whole() && lr_full_on(ctx)) UCHK(enqueue_full_lr(ctx, s, si, d_out[0]));
    return r.full ? enqueue_prolong(ctx, s, si, r.to, d_out, r.full) : UGSM_OK;
}

// The seeded full-mode call (ugsm_submit_full_seeded; its refusals: ugsm_seeded.cpp): n pairs in lockstep from level `start_level` of their priors.
int seeded_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                        const float *const *d_prior, int start_level, float *const *d_out)
{
    return submit_pairs(ctx, slot, n, batch_runs_pair_by_pair(ctx) ? 1 : n, [&](Slot &s, int b, int k) {
        const LevelRange r = LevelRange::seeded(start_level, d_prior + b);
        return enqueue_match_full(ctx, s, slot, k, d_rgbL + b, d_rgbR + b, W, H, stride, d_out + b, &r);
    });
}

// The full-mode call in two halves (ugsm_submit_full_coarse, ugsm_submit_full_fine; their refusals: ugsm_coarse.cpp), n pairs in lockstep.
// Coarse: the levels top .. stop_level into d_state, and the prolongation.  Fine: the levels state_level - 1 .. 0 from the states of state_level.
int coarse_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                        int stop_level, float *const *d_state, float *const *d_full)
{
    return submit_pairs(ctx, slot, n, batch_runs_pair_by_pair(ctx) ? 1 : n, [&](Slot &s, int b, int k) {
        const LevelRange r = LevelRange::coarse(ctx->cfg.levels, stop_level, d_full ? d_full + b : nullptr);
        return enqueue_match_full(ctx, s, slot, k, d_rgbL + b, d_rgbR + b, W, H, stride, d_state + b, &r);
    });
}
int fine_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                      const float *const *d_state, int state_level, float *const *d_out)
{
    return submit_pairs(ctx, slot, n, batch_runs_pair_by_pair(ctx) ? 1 : n, [&](Slot &s, int b, int k) {
        const LevelRange r = LevelRange::fine(state_level, d_state + b);
        return enqueue_match_full(ctx, s, slot, k, d_rgbL + b, d_rgbR + b, W, H, stride, d_out + b, &r);
    });
}

// What ugsm_submit_full_checked and ugsm_match_full_checked refuse before anything is enqueued, beyond their null pointers.  The threshold is
// the call's own: the context's setting (ugsm_set_lr_check) is neither read nor changed.
int full_checked_check(ugsm_ctx *ctx, int n, int W, int H, int stride, float tau)
{
    if (n < 1 || n > UGSM_MAX_BATCH) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked full-mode call takes 1 .. UGSM_MAX_BATCH pairs");
    if (!(tau > 0.0f)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked full-mode call needs tau > 0");
    // (ugsm_set_lr_check's rule: these contexts run every level pair by pair and have no batch dimension to carry the second direction in)
    if (ctx->cfg.early_exit_threshold > 0.0f || ctx->cfg.kernel_path == 1)
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked full-mode call: not with early_exit_threshold > 0 or kernel_path 1");
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));
    UCHK(input_status(ctx, W, stride));
    return UGSM_OK;
}
// ... and its buffers: A, d0 and d1 for 2 n full fields, the LR buffer for the `kept` right-to-left fields the caller does not take and the
// count words.  A buffer that cannot grow answers UGSM_ERR_NOMEM here, before anything is enqueued (ensure_level_bufs: all or nothing).
int full_checked_bufs(ugsm_ctx *ctx, Slot &s, int n, int kept, int W, int H)
{
    const size_t field = field_room((size_t)W * H);  // (Slot::lvl_stride, as prepare_slot sets it for this size)
    UCHK(ensure_level_bufs(ctx, s, 2 * (size_t)n * field));
    return lr_ready(ctx, s, lr_full_room(field, kept, n));
}

// ---- the queue's checked pairs (ugsm_enqueue_full_checked*; CtxHooks::checked_submit / checked_marked) ------------------------------------
// A call of n checked pairs is ONE slot-level checked call: ugsm_submit_full_checked on the device kind's buffers, ugsm_submit_full_checked_host
// on a managed call's page-locked staging; pairs that carry a cloud go through the cloud call's frame (ugsm_cloud.cpp).
int queue_checked_submit(ugsm_ctx *ctx, int slot, const CheckedCall *call)
{
    if (!call || call->n < 1 || call->n > UGSM_MAX_BATCH) return UGSM_ERR_BAD_ARG;
    if (call->spec) return queue_checked_cloud_submit(ctx, slot, call);
    const int n = call->n;
    const uint8_t *L[UGSM_MAX_BATCH], *R[UGSM_MAX_BATCH];
    float *out[3][UGSM_MAX_BATCH], *back[3][UGSM_MAX_BATCH];
    bool any_back = false;
    for (int b = 0; b < n; b++) {
        const CheckedJob &j = call->job[b];
        L[b] = j.L;
        R[b] = j.R;
        for (int k = 0; k < 3; k++) {
            out[k][b] = call->managed ? j.planes[k] : (k == 0 ? j.out : nullptr);
            back[k][b] = call->managed ? j.back_planes[k] : (k == 0 ? j.back : nullptr);
        }
        any_back = any_back || back[0][b];
    }
    if (!call->managed)
        return ugsm_submit_full_checked(ctx, slot, n, L, R, call->W, call->H, call->stride, out[0], any_back ? back[0] : nullptr, call->tau);
    return ugsm_submit_full_checked_host(ctx, slot, n, L, R, call->W, call->H, call->stride, out[0], out[1], out[2], any_back ? back[0] : nullptr,
                                         any_back ? back[1] : nullptr, any_back ? back[2] : nullptr, call->tau);
}
int queue_checked_marked(ugsm_ctx *ctx, int slot, int n, long long *fwd, long long *back)
{
    for (int b = 0; b < n; b++) UCHK(ugsm_last_lr_marked_pair(ctx, slot, b, fwd + b, back + b));
    return UGSM_OK;
}

}  // namespace ugsm

extern "C" {

int ugsm_submit_full(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_out) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(enqueue_match_full(ctx, *s, slot, 1, &d_rgbL, &d_rgbR, W, H, stride, &d_out));
    return mark_done(ctx, *s);
}

// ---- B pairs per call ---------------------------------------------------------------------------------------------------------
int ugsm_submit_full_batch(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                           float *const *d_out)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (n < 1 || n > UGSM_MAX_BATCH || !d_rgbL || !d_rgbR || !d_out) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < n; b++)
        if (!d_rgbL[b] || !d_rgbR[b] || !d_out[b]) return UGSM_ERR_BAD_ARG;
    const int per = batch_runs_pair_by_pair(ctx) ? 1 : n;  // pairs per match: one by one, or all in lockstep
    return submit_pairs(ctx, *s, n, per, [&](Slot &sl, int b, int k) { return enqueue_match_full(ctx, sl, slot, k, d_rgbL + b, d_rgbR + b, W, H, stride, d_out + b); });
}

// ---- both directions of n full-mode pairs -------------------------------------------------------------------------------------
int ugsm_submit_full_checked(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                             float *const *d_out, float *const *d_back, float tau)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_rgbL || !d_rgbR || !d_out) return UGSM_ERR_BAD_ARG;
    UCHK(full_checked_check(ctx, n, W, H, stride, tau));
    int kept = 0;
    for (int b = 0; b < n; b++) {
        if (!d_rgbL[b] || !d_rgbR[b] || !d_out[b]) return UGSM_ERR_BAD_ARG;
        kept += !(d_back && d_back[b]);
    }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(full_checked_bufs(ctx, *s, n, kept, W, H));
    UCHK(enqueue_full_checked(ctx, *s, slot, n, d_rgbL, d_rgbR, W, H, stride, d_out, d_back, tau));
    return mark_done(ctx, *s);
}

}  // extern "C"
