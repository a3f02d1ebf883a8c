// ugsm_fovea.cpp -- the foveated calls.  First the steps: the windows of a call's pairs, the fine phase (matching() with foveatedmatching == 1
// below level F-1), the stack check, the restriction from priors, level 0 inside several windows.  Then the one sequence made of them
// (enqueue_foveated), which every kind of call -- pairs, with the LR check in lockstep, several windows on one pair and their checked form, warm
// from a prior -- goes through as a FoveaCall, with the one function that grows its buffers (fovea_grow).  The coarse phase is the full-frame
// descent stopped at level F-1 (enqueue_fovea_coarse, ugsm_full.cpp); the levels' own work is ugsm_levels.cpp.  At the end the ugsm_submit_*
// entry points of the family, and hierarchicalDisparity over the stacks.
#include "ugsm_slot.hpp"

#include <algorithm>

using namespace ugsm;

namespace ugsm {
namespace {

// the windows of a foveated call's pairs (n offsets), for enqueue_pyramids
int fovea_windows(const ugsm_ctx *ctx, int W, int H, int n, const int *off_x, const int *off_y, FoveaWin &win)
{
    const int F = ctx->cfg.fovea_levels;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));
    if (F < 2 || F > ctx->cfg.levels || n < 1 || n > kMaxBatch) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < n; b++) {
        FoveaGeom g;
        fovea_geometry(w, h, F, off_x[b], off_y[b], g);
        win.w = g.fw;
        win.h = g.fh;
        win.x0[b] = g.ox[0];
        win.y0[b] = g.oy[0];
    }
    return UGSM_OK;
}

// The fine phase for the sh.nb entries of the call: per-entry states and stacks (sh.nb of each), and sh.nreal window offsets and pyramid-stack
// destinations (d_pyrL / d_pyrR may be null, and so may their entries): an exchanged entry of a shape of both directions has its twin's window,
// and the pyramid stacks are the real pairs'.
// first (the warm call, ugsm_submit_foveated_warm; < 0: none): the levels first .. 0 only, from starting fields that the caller's launch has
// put where d_state is otherwise copied to -- s.d0, entry b at + b * sh.stride --: d_state is not read, the row blocks above `first` are the
// caller's, and level `first` takes no seed.  first == F-1: the whole level F-1 is matched first, as the last level of the coarse phase is but
// never as a top level (a prior has a confidence), and its block follows.
int enqueue_fovea_fine(ugsm_ctx *ctx, Slot &s, int si, const Shape &sh, const float *const *d_state, const int *off_x, const int *off_y,
                       float *const *d_stack, float *const *d_pyrL, float *const *d_pyrR, int first = -1)
{
    const int levels = s.levels, F = ctx->cfg.fovea_levels, nb = sh.nb;
    if (F < 2 || F > levels || first >= F) return UGSM_ERR_BAD_ARG;
    FoveaGeom g[2 * kMaxBatch];
    for (int b = 0; b < nb; b++) fovea_geometry(s.w, s.h, F, off_x[b % sh.nreal], off_y[b % sh.nreal], g[b]);
    const int fw = g[0].fw, fh = g[0].fh;
    const size_t fn = (size_t)fw * fh;
    const int np = launch_pairs(ctx, sh, fw, fh);  // (every level of the fine phase is a window of this size)
    float *cur = s.d0, *other = s.d1;
    for (int b = 0; first < 0 && b < nb; b++)
        HIPCHK(ctx, hipMemcpyAsync(cur + b * sh.stride, d_state[b], sizeof(float) * 3 * fn, hipMemcpyDeviceToDevice, s.st));
    // a stack row block / a pyramid-stack block for every entry: one launch for the batch
    auto copy_out = [&](int pairs, const Img3 *views, const float *field, float *const *dsts, size_t dst_off, size_t dst_plane) {
        for_groups(pairs, np > 1, [&](Grp gr) {
            const Batch bt = copy_batch(sh, gr, views, dsts, dst_off);
            const Img3 src = views ? views[gr.b0] : Img3{field + gr.b0 * sh.stride, fw, fn};
            launch_copy_view(s.st, src, fw, fh, dsts[gr.b0] + dst_off, dst_plane, fw, gr.n > 1 ? &bt : nullptr);
        });
    };
    // stack row block F-1 = the whole level F-1 (UG_GPU_matcher.cpp:293-303)
    if (first < 0) copy_out(nb, nullptr, cur, d_stack, (size_t)(F - 1) * fn, (size_t)F * fn);
    SeedMap sm[2 * kMaxBatch];
    Img3 Lv[2 * kMaxBatch], Rv[2 * kMaxBatch];
    for (int i = first < 0 ? F - 2 : first; i >= 0; i--) {
        s.cur_level = i;
        for (int b = 0; b < nb; b++) {
            const int ox = i < F - 1 ? g[b].ox[i] : 0, oy = i < F - 1 ? g[b].oy[i] : 0;
            Lv[b] = level_view(s, pair_pyr(s, sh, 0, b), i, ox, oy);
            Rv[b] = level_view(s, pair_pyr(s, sh, 1, b), i, ox, oy);
        }
        const bool seeded = i != first && hand_seed(ctx, s, si, sh, fw, fh, fw, fh, g, i, sm, cur, other);
        const int mi = level_iterations(i);
        UCHK(run_level(ctx, s, si, sh, Lv, Rv, fw, fh, mi, level_smooth(i), false, 1, mi, cur, other, nullptr, nullptr, seeded ? sm : nullptr));
        copy_out(nb, nullptr, cur, d_stack, (size_t)i * fn, (size_t)F * fn);
    }
    // pyramid stacks as the node publishes them (UG_GPU_matcher.cpp:203-213): [level][channel][row]
    for (int side = 0; side < 2; side++) {
        float *const *dsts = side == 0 ? d_pyrL : d_pyrR;
        if (!dsts) continue;
        const int nr = sh.nreal;
        bool all = true, any = false;
        for (int b = 0; b < nr; b++) {
            all = all && dsts[b] != nullptr;
            any = any || dsts[b] != nullptr;
        }
        if (!any) continue;
        const float *pyr = side == 0 ? s.pyrL : s.pyrR;
        for (int k = 0; k < F; k++) {
            for (int b = 0; b < nr; b++) {
                const int ox = (k < F - 1) ? g[b].ox[k] : 0, oy = (k < F - 1) ? g[b].oy[k] : 0;
                Lv[b] = level_view(s, pyr + b * s.pyr_stride, k, ox, oy);
            }
            if (all) {
                copy_out(nr, Lv, nullptr, dsts, (size_t)k * 3 * fn, fn);
            } else {
                for (int b = 0; b < nr; b++)
                    if (dsts[b]) launch_copy_view(s.st, Lv[b], fw, fh, dsts[b] + (size_t)k * 3 * fn, fn, fw);
            }
        }
    }
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

// The room a checked foveated call takes in the slot's LR buffer, in floats.  Entry k's right-to-left stack lies at k * per; the count words (one
// of 8 bytes per (entry, level); at a multiple of 64 floats: aligned) at cnt.  The right-to-left level-F-1 state: n pairs keep one each behind
// their stack, at k * per + state; n windows of one pair (one_state) share one behind the last stack, at state.
struct LrRoom {
    size_t per, state, cnt, total;
};
LrRoom lr_room(int n, int F, int fw, int fh, bool one_state)
{
    const size_t stackf = 3 * (size_t)F * fw * fh, field = 3 * (size_t)fw * fh;
    LrRoom r;
    r.per = ((one_state ? stackf : stackf + field) + 63) & ~(size_t)63;
    r.state = one_state ? (size_t)n * r.per : stackf;
    r.cnt = (size_t)n * r.per + (one_state ? field_room((size_t)fw * fh) : 0);
    r.total = r.cnt + 2 * (size_t)n * F;
    return r;
}

// The tail of a checked foveated call: one launch of k_lr_check's stack form over every level of the n stacks against their right-to-left
// twins (entry k's at s.lr + k * per) -- after the last level, so nothing feeds back into the matching -- and the counts back with one copy on
// the slot's stream.
int enqueue_lr_stack_check(ugsm_ctx *ctx, Slot &s, int si, int n, int F, int fw, int fh, float tau, float *const *d_stack, size_t per,
                           unsigned long long *cnt)
{
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof *cnt * n * F, s.st));
    LrStack ls{};
    ls.n = n;
    ls.F = F;
    for (int b = 0; b < n; b++) {
        ls.fwd[b] = byte_diff(d_stack[b], d_stack[0]);
        ls.back[b] = (long long)((size_t)b * per * sizeof(float));
    }
    {
        Timer t(ctx, &s, si, KC_MISC, (double)((size_t)fw * fh) * F * n);
        launch_lr_check(s.st, d_stack[0], s.lr, fw, fh, tau, cnt, ls);
    }
    HIPCHK(ctx, hipMemcpyAsync(s.lr_host + 1, cnt, sizeof *cnt * n * F, hipMemcpyDeviceToHost, s.st));
    HIPCHK(ctx, hipGetLastError());
    s.lr_fov_pairs = n;
    s.lr_fov_F = F;
    return UGSM_OK;
}

// (single pairs: the stage-wise entry points, and a multi-window call that runs window by window)
int enqueue_fovea_coarse(ugsm_ctx *ctx, Slot &s, int si, float *d_state) { return enqueue_fovea_coarse(ctx, s, si, Shape::pairs(s), &d_state); }
int enqueue_fovea_fine(ugsm_ctx *ctx, Slot &s, int si, const float *d_state, int off_x, int off_y, float *d_stack, float *d_pyrL, float *d_pyrR)
{
    return enqueue_fovea_fine(ctx, s, si, Shape::pairs(s), &d_state, &off_x, &off_y, &d_stack, d_pyrL ? &d_pyrL : nullptr, d_pyrR ? &d_pyrR : nullptr);
}

}  // namespace

// The starting fields of the fovea levels start .. F-1 of n entries from their priors, one launch (launch_restrict_stack): the rows from the
// two windows' geometries; up to kRestrictStackByValue of them in the launch's arguments, more through the slot's table.  Level `start` goes
// to `work` (entry b at + b * work_stride floats) where that is given, everything else to the row blocks of d_stack.
int enqueue_restrict_stack(ugsm_ctx *ctx, Slot &s, int si, int n, const int *w, const int *h, int F, const float *const *prior, const int *poff_x,
                           const int *poff_y, bool field, const int *off_x, const int *off_y, int start, float *const *d_stack, float *work, size_t work_stride)
{
    RestrictStack rs{};
    rs.n = n;
    rs.F = F;
    rs.s = start;
    rs.field = field ? 1 : 0;
    rs.W = w[0];
    rs.H = h[0];
    rs.fw = w[F - 1];
    rs.fh = h[F - 1];
    for (int l = 0; l < F; l++) {
        rs.w[l] = w[l];
        rs.h[l] = h[l];
    }
    RestrictStackRow local[kRestrictStackByValue], *rows = local;
    const bool table = n > kRestrictStackByValue;
    if (table) UCHK(s.warm.begin(ctx, s.st, (size_t)kMaxBatch, &rows));
    for (int b = 0; b < n; b++) {
        FoveaGeom gn, gp;
        fovea_geometry(w, h, F, off_x ? off_x[b] : 0, off_y ? off_y[b] : 0, gn);
        if (!field) fovea_geometry(w, h, F, poff_x ? poff_x[b] : 0, poff_y ? poff_y[b] : 0, gp);
        RestrictStackRow &r = rows[b];
        r = RestrictStackRow{};
        r.prior = byte_diff(prior[b], prior[0]);
        r.dst = byte_diff(d_stack[b], d_stack[0]);
        r.work = (long long)(b * work_stride * sizeof(float));
        for (int l = 0; l < F - 1; l++) {
            r.nox[l] = gn.ox[l];
            r.noy[l] = gn.oy[l];
            r.pox[l] = field ? 0 : gp.ox[l];
            r.poy[l] = field ? 0 : gp.oy[l];
        }
    }
    if (table) {
        UCHK(s.warm.upload(ctx, s.st, (size_t)n));
        rs.table = s.warm.tab;
    }
    s.cur_level = start;
    bool ok;
    {
        Timer t(ctx, &s, si, KC_RESTRICT_STACK, (double)n * (F - start) * rs.fw * rs.fh);
        ok = launch_restrict_stack(s.st, prior[0], d_stack[0], work, rs, rows);
    }
    s.cur_level = kNoLevel;
    if (!ok) return ctx_fail(ctx, UGSM_ERR_STATE, "the warm foveated call: a window that leaves its level");
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

// Level 0 of both images inside the n windows of a multi-window call (k_pyr_base stored none: FoveaWin::later), one launch.
static int enqueue_level0_windows(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int stride, int n, const FoveaWin &win)
{
    if (ctx->cfg.kernel_path != 1 && s.levels >= 3) {  // (k_pyr_base built them: as `base` in build_pyramids)
        Level0Windows lw{};
        lw.n = n;
        lw.w = win.w;
        lw.h = win.h;
        for (int k = 0; k < n; k++) {
            lw.x0[k] = win.x0[k];
            lw.y0[k] = win.y0[k];
        }
        s.cur_level = 0;
        bool ok;
        {
            Timer t(ctx, &s, si, KC_LEVEL0_WIN, 2.0 * n * win.w * win.h);
            ok = launch_level0_windows(s.st, d_rgbL, d_rgbR, stride, s.W, s.H, s.pyrL + s.off[0], s.pyrR + s.off[0], lw, ctx->hooks.input_format);
        }
        s.cur_level = kNoLevel;
        if (!ok) {
            ctx->err = "a fovea window leaves the frame";
            return UGSM_ERR_STATE;
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return UGSM_OK;
}

// ---- the foveated call ------------------------------------------------------------------------------------------------------------------
// A call runs checked -- both directions in lockstep, the stacks checked against their right-to-left twins -- with the threshold it brings, and a
// call of pairs under the context's own setting (ugsm_set_lr_check) too.
static float checked_tau(const ugsm_ctx *ctx, const FoveaCall &call)
{
    return call.tau > 0.0f ? call.tau : (call.kind == FoveaCall::Pairs && lr_fovea_on(ctx)) ? ctx->lr_tau : 0.0f;
}

// The sizes of a foveated call of the context on W x H images, and the states of n pairs / n windows of one pair at the front of hout.
int fovea_room(const ugsm_ctx *ctx, int W, int H, FoveaCall::Kind kind, int n, FoveaRoom &room)
{
    const int F = ctx->cfg.fovea_levels;
    room = FoveaRoom{};
    UCHK(ugsm_fovea_dims(W, H, ctx->cfg.levels, F, &room.fw, &room.fh));
    room.px = (size_t)room.fw * room.fh;
    room.field = field_room(room.px);
    room.plane = (size_t)F * room.px;
    room.stack = 3 * room.plane;
    room.total = (kind == FoveaCall::Pairs ? n : kind == FoveaCall::Windows ? 1 : 0) * room.field;
    return UGSM_OK;
}

// Everything the call needs beyond its pairs' own buffers (prepare_slot), grown before anything is enqueued: a refused call has enqueued nothing.
//   - the level buffers for the windows of one pair, whose fields run in lockstep at a stride of one fovea field: n of them (2 n checked) exceed the
//     one pair's 3 W H floats as soon as n > 2^(F-1).  Never less than 3 W H, so that prepare_slot need not grow them again.  (Both directions of n
//     PAIRS fit into what prepare_slot gives n pairs -- fovW fovH <= W H / 2 for every F >= 2, for F = 2 just --: enqueue_foveated sees to the
//     rounding behind the pyramids, where the slot has its size);
//   - a checked call's LR buffer (lr_room) and the page-locked words its counts come back in.  What does NOT fit into the level buffers for F = 2 is
//     the right-to-left STACK, which has to outlive the fine levels: it goes there, with the right-to-left state -- 3 (F + 1) fovW fovH floats per
//     pair, 24 MB at 16 MP beside the pair's 1.35 GB, counted by ugsm_context_device_bytes;
//   - hout, for the states and what the entry point has asked for behind them.
int fovea_grow(ugsm_ctx *ctx, Slot &s, int W, int H, const FoveaCall &call, const FoveaRoom &room)
{
    const bool windows = call.kind == FoveaCall::Windows, checked = checked_tau(ctx, call) > 0.0f;
    if (windows && (checked || !fovea_windows_run_one_by_one(ctx, call.n)))
        UCHK(ensure_level_bufs(ctx, s, std::max((checked ? 2 : 1) * call.n * room.field, 3 * (size_t)W * H)));
    if (checked) UCHK(lr_ready(ctx, s, lr_room(call.n, ctx->cfg.fovea_levels, room.fw, room.fh, windows).total));
    return s.hout.grow(ctx, room.total);
}

// One foveated call on device buffers, every kind of it (FoveaCall; d_rgbL / d_rgbR: the n pairs' images, or the one pair's).  The steps are the
// same for all; what differs is data -- kind: A planes from the side stream | level 0 | coarse phase on | fine phase on | range word | level-F-1 states:
//   pairs:            F-1 .. top if n == 1 (a batch computes A in line) | k_pyr_base, inside the windows | Shape::pairs | Shape::pairs | -- | n
//   pairs, checked:   none | same | Shape::both_directions | the same shape | words 0 .. n-1 copied to n .. 2n-1 | n, and n behind the twins' stacks in the LR buffer
//   windows:          F-1 .. top | none from k_pyr_base (FoveaWin::later), then one k_level0_windows launch | one pair | Shape::windows in lockstep, or window
//                     by window (fovea_windows_run_one_by_one) | word 0 doubled out to n entries | 1
//   windows, checked: none | as windows | Shape::coarse_both_directions | Shape::windows_both_directions | word 0 doubled out to 2n | 1, and 1 behind the last twin stack
//   warm:             none; the pyramids stop at max(start, 2) | inside the windows | not run: one k_restrict_stack launch | Shape::pairs, from level `start` | -- | none
//   - an exchanged entry (n + b of a checked call) reads its pair's pyramids with the L and R views exchanged (pair_pyr), through entry b's windows
//     and seed maps, under its pair's range word (it covers both images' pyramids: build_pyramids reports either image into range_bad[pair]), so
//     nothing more is stored for the second direction.  Every kernel of a level takes the entries in one launch except K-cost, which takes each
//     direction in one (run_level); more than kMaxBatch entries go through launches of equal size (group_pairs);
//   - the windows of one pair share what does not depend on the window: the pyramids, the coarse phase and its state.  Pyramids that k_pyr_base does
//     not build (fewer than three levels, kernel_path 1) hold level 0 whole and skip the k_level0_windows launch;
//   - a warm call (its refusals: ugsm_fovea_seeded.cpp) computes A in line at every level, level F-1 included, where it is matched: the side stream's
//     A planes serve the coarse phase.  The one launch writes level `start`'s fields into the level buffer the fine phase starts in, the levels
//     above into the stacks' row blocks;
// Afterwards the slot holds no whole pyramids (have_pyr false: every foveated call builds them through its windows).
int enqueue_foveated(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride, const FoveaCall &call)
{
    const int F = ctx->cfg.fovea_levels, n = call.n;
    const bool windows = call.kind == FoveaCall::Windows, warm = call.kind == FoveaCall::Warm;
    const float tau = checked_tau(ctx, call);
    const bool checked = tau > 0.0f;
    FoveaWin win;
    UCHK(fovea_windows(ctx, W, H, n, call.off_x, call.off_y, win));
    win.later = windows;
    FoveaRoom room;
    UCHK(fovea_room(ctx, W, H, call.kind, n, room));
    UCHK(fovea_grow(ctx, s, W, H, call, room));

    const bool side_A = !checked && !warm && (windows || n == 1);
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, windows ? 1 : n, W, H, stride, side_A ? F - 1 : -1, &win, false, 0, warm ? call.start : -1));
    if (windows) UCHK(enqueue_level0_windows(ctx, s, si, d_rgbL[0], d_rgbR[0], stride, n, win));

    // what runs in lockstep: the real pairs, unless the call is checked or its windows run together
    const bool one_by_one = windows && !checked && fovea_windows_run_one_by_one(ctx, n);
    const Shape real = Shape::pairs(s);
    Shape coarse = real, fine = real;
    if (checked && !windows) coarse = fine = Shape::both_directions(n, room.field);
    if (checked && windows) { coarse = Shape::coarse_both_directions(room.field); fine = Shape::windows_both_directions(n, room.field); }
    if (!checked && windows && !one_by_one) fine = Shape::windows(n, room.field);
    // The slot has its size now, and prepare_slot may have given the level buffers back and sized them for this call's pairs alone (the
    // configured batch did not fit): checked pairs grow them to their 2 n fields where the rounding asks for it, the windows' fields are refused
    const LrRoom lr = lr_room(n, F, room.fw, room.fh, windows);
    if (checked && !windows) UCHK(ensure_level_bufs(ctx, s, fine.nb * fine.stride));
    if (windows && !one_by_one && (fine.nb * fine.stride > s.lvl_cap || (checked && (lr.total > s.lr.cap || !s.lr_host))))
        return ctx_fail(ctx, UGSM_ERR_STATE, checked ? "the slot's buffers do not hold the checked windows' fields" : "the level buffers do not hold the windows' fields");
    // the range words of the real pairs (the one pair of n windows) out to the entries that run under them, doubling what is already there
    for (int c = windows ? 1 : n; s.range_known && c < fine.nb; c *= 2)
        HIPCHK(ctx, hipMemcpyAsync(s.range_bad + c, s.range_bad, sizeof(unsigned) * std::min(c, fine.nb - c), hipMemcpyDeviceToDevice, s.st));

    // entry b's state and stack, and its twin's (entry n + b) in the LR buffer: n pairs keep a state each, n windows share one
    float *state[2 * kMaxBatch] = {}, *stack[2 * kMaxBatch] = {};
    for (int b = 0; b < n; b++) {
        if (!warm) state[b] = s.hout + (windows ? 0 : b * room.field);
        stack[b] = call.d_stack[b];
        if (!checked) continue;
        stack[n + b] = s.lr + b * lr.per;
        state[n + b] = s.lr + lr.state + (windows ? 0 : b * lr.per);
    }
    if (warm) {
        UCHK(enqueue_restrict_stack(ctx, s, si, n, s.w, s.h, F, call.d_prior, call.prior_off_x, call.prior_off_y, call.field, call.off_x, call.off_y,
                                    call.start, call.d_stack, s.d0, real.stride));
    } else {
        float *const both[2] = {state[0], state[n]};  // (the windows' coarse phase: the one pair, and its twin)
        UCHK(enqueue_fovea_coarse(ctx, s, si, coarse, windows ? both : state));
    }
    // (windows that run one by one: `fine` is the one real pair, window k after window k - 1 from the one state)
    for (int k = 0; k < (one_by_one ? n : 1); k++)
        UCHK(enqueue_fovea_fine(ctx, s, si, fine, warm ? nullptr : state, call.off_x + k, call.off_y + k, stack + k, call.d_pyrL, call.d_pyrR, warm ? call.start : -1));
    if (!checked) return UGSM_OK;
    return enqueue_lr_stack_check(ctx, s, si, n, F, room.fw, room.fh, tau, call.d_stack, lr.per, reinterpret_cast<unsigned long long *>(s.lr + lr.cnt));
}

int fovea_warm_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride, const int *off_x,
                      const int *off_y, const float *const *d_prior, const int *prior_off_x, const int *prior_off_y, int field, int start_level,
                      float *const *d_stack)
{
    const FoveaCall call = FoveaCall::warm(n, off_x, off_y, d_prior, prior_off_x, prior_off_y, field != 0, start_level, d_stack);
    const int per = (n == 1 || fovea_batch_runs_pair_by_pair(ctx)) ? 1 : n;  // (kernel_path 1: the pairs one after the other, as ugsm_submit_foveated_batch)
    return submit_pairs(ctx, slot, n, per, [&](Slot &s, int b, int k) { return enqueue_foveated(ctx, s, slot, d_rgbL + b, d_rgbR + b, W, H, stride, call.sub(b, k)); });
}

// ---- n windows on one pair ----------------------------------------------------------------------------------------------------
// What ugsm_submit_foveated_multi and ugsm_match_foveated_multi refuse before anything is enqueued.
// tau: null = the plain call; else the checked call's threshold (ugsm_submit_foveated_multi_checked), which has refusals of its own and does
// not look at the context's setting.
int multi_check(ugsm_ctx *ctx, int n, int W, int H, int stride, const float *tau)
{
    const int F = ctx->cfg.fovea_levels;
    if (n < 1 || n > UGSM_MAX_BATCH || F < 2) return UGSM_ERR_BAD_ARG;
    if (tau && !(*tau > 0.0f)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked multi-window call needs tau > 0");
    // (ugsm_set_lr_check's rule: these contexts run every level pair by pair and have no batch dimension to carry the second direction in)
    if (tau && (ctx->cfg.early_exit_threshold > 0.0f || ctx->cfg.kernel_path == 1))
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked multi-window call: not with early_exit_threshold > 0 or kernel_path 1");
    if (!tau && lr_fovea_on(ctx)) return ctx_fail(ctx, UGSM_ERR_STATE, "the foveated LR check is on: the checked multi-window call is ugsm_submit_foveated_multi_checked (ugsm_set_lr_check)");
    int fw, fh;
    UCHK(ugsm_fovea_dims(W, H, ctx->cfg.levels, F, &fw, &fh));
    UCHK(input_status(ctx, W, stride));
    return UGSM_OK;
}

}  // namespace ugsm

extern "C" {

int ugsm_submit_pyramids(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    // (no A planes here: the ranks of a fovea shard that only run the fine phase never use them; a coarse phase that follows computes
    // them on the side stream itself -- ADVICE r03)
    UCHK(enqueue_pyramids(ctx, *s, slot, d_rgbL, d_rgbR, W, H, stride, -1));
    return mark_done(ctx, *s);
}

int ugsm_submit_fovea_coarse(ugsm_ctx *ctx, int slot, float *d_state)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_state) return UGSM_ERR_BAD_ARG;
    if (!s->have_pyr) return UGSM_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (s->a_from < 0 && side_stream_ok(ctx, *s) && ctx->cfg.fovea_levels >= 2) UCHK(enqueue_side_A(ctx, *s, ctx->cfg.fovea_levels - 1));
    UCHK(enqueue_fovea_coarse(ctx, *s, slot, d_state));
    return mark_done(ctx, *s);
}

int ugsm_submit_fovea_fine(ugsm_ctx *ctx, int slot, const float *d_state, int off_x, int off_y, float *d_stack)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_state || !d_stack) return UGSM_ERR_BAD_ARG;
    if (!s->have_pyr) return UGSM_ERR_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(enqueue_fovea_fine(ctx, *s, slot, d_state, off_x, off_y, d_stack, nullptr, nullptr));
    return mark_done(ctx, *s);
}

int ugsm_submit_foveated(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride,
                         int off_x, int off_y, float *d_stack, float *d_pyrL, float *d_pyrR)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_stack) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (ctx->cfg.fovea_levels < 2) return UGSM_ERR_BAD_ARG;
    UCHK(enqueue_foveated(ctx, *s, slot, &d_rgbL, &d_rgbR, W, H, stride, FoveaCall::pairs(1, &off_x, &off_y, &d_stack, &d_pyrL, &d_pyrR)));
    return mark_done(ctx, *s);
}

int ugsm_submit_foveated_batch(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                               const int *off_x, const int *off_y, float *const *d_stack, float *const *d_pyrL, float *const *d_pyrR)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (n < 1 || n > UGSM_MAX_BATCH || !d_rgbL || !d_rgbR || !d_stack) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < n; b++)
        if (!d_rgbL[b] || !d_rgbR[b] || !d_stack[b]) return UGSM_ERR_BAD_ARG;
    if (ctx->cfg.fovea_levels < 2) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const FoveaCall call = FoveaCall::pairs(n, off_x, off_y, d_stack, d_pyrL, d_pyrR);
    FoveaRoom room;
    UCHK(fovea_room(ctx, W, H, call.kind, n, room));
    UCHK(fovea_grow(ctx, *s, W, H, call, room));  // (the whole call's, whichever way it runs)
    const int per = (n == 1 || fovea_batch_runs_pair_by_pair(ctx)) ? 1 : n;
    for (int b = 0; b < n; b += per) UCHK(enqueue_foveated(ctx, *s, slot, d_rgbL + b, d_rgbR + b, W, H, stride, call.sub(b, per)));
    return mark_done(ctx, *s);
}

// (tau: null = the plain call, else the checked one's threshold)
static int submit_foveated_multi(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int n, const int *off_x,
                                 const int *off_y, float *const *d_stack, const float *tau)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_rgbL || !d_rgbR || !d_stack) return UGSM_ERR_BAD_ARG;
    for (int k = 0; k < n && k < UGSM_MAX_BATCH; k++)
        if (!d_stack[k]) return UGSM_ERR_BAD_ARG;
    UCHK(multi_check(ctx, n, W, H, stride, tau));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const FoveaCall call = FoveaCall::windows(n, off_x, off_y, d_stack);
    UCHK(enqueue_foveated(ctx, *s, slot, &d_rgbL, &d_rgbR, W, H, stride, tau ? call.checked(*tau) : call));
    return mark_done(ctx, *s);
}

int ugsm_submit_foveated_multi_checked(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int n,
                                       const int *off_x, const int *off_y, float *const *d_stack, float tau)
{
    return submit_foveated_multi(ctx, slot, d_rgbL, d_rgbR, W, H, stride, n, off_x, off_y, d_stack, &tau);
}

int ugsm_submit_foveated_multi(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int n,
                               const int *off_x, const int *off_y, float *const *d_stack)
{
    return submit_foveated_multi(ctx, slot, d_rgbL, d_rgbR, W, H, stride, n, off_x, off_y, d_stack, nullptr);
}

// hierarchicalDisparity, MatchGPULib.cpp:2589-2701
int ugsm_reconstruct_full(ugsm_ctx *ctx, int slot, const float *d_stackH, const float *d_stackV, const float *d_stackC, int W, int H,
                          int off_x, int off_y, float *d_out3)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_stackH || !d_stackV || !d_stackC || !d_out3) return UGSM_ERR_BAD_ARG;
    const int levels = ctx->cfg.levels, F = ctx->cfg.fovea_levels;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, levels, w, h));
    if (F < 1 || F > levels) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    FoveaGeom g;
    if (F >= 2) fovea_geometry(w, h, F, off_x, off_y, g);
    else { g.fw = w[0]; g.fh = h[0]; }
    const size_t fl = (size_t)g.fw * g.fh;
    if (F == 1) {  // the stack is the full frame already
        const float *src[3] = {d_stackH, d_stackV, d_stackC};
        for (int c = 0; c < 3; c++) HIPCHK(ctx, hipMemcpyAsync(d_out3 + c * fl, src[c], fl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
        return UGSM_OK;
    }
    UCHK(ensure_level_bufs(ctx, *s, 3 * (size_t)w[1] * h[1]));
    // level F-1 (whole frame) as a 3-plane field
    float *cur = s->d0, *other = s->d1;
    {
        const float *src[3] = {d_stackH, d_stackV, d_stackC};
        for (int c = 0; c < 3; c++)
            HIPCHK(ctx, hipMemcpyAsync(cur + c * fl, src[c] + (size_t)(F - 1) * fl, fl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    }
    for (int level = F - 1; level > 0; level--) {
        float *dst = (level == 1) ? d_out3 : other;
        Timer t(ctx, s, slot, KC_MISC, (double)w[level - 1] * h[level - 1]);
        launch_upsample_paste(s->st, cur, w[level], h[level], dst, w[level - 1], h[level - 1], d_stackH + (size_t)(level - 1) * fl,
                              d_stackV + (size_t)(level - 1) * fl, d_stackC + (size_t)(level - 1) * fl, g.fw, g.fh, g.ox[level - 1], g.oy[level - 1]);
        std::swap(cur, other);
    }
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

// hierarchicalDisparity over the stacks of n windows of one pair: the steps of ugsm_reconstruct_full, every one pasting all the windows
int ugsm_reconstruct_full_multi(ugsm_ctx *ctx, int slot, int n, const float *const *d_stack, int W, int H, const int *off_x, const int *off_y,
                                float *d_out3)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_stack || !d_out3 || n < 1 || n > UGSM_MAX_BATCH) return UGSM_ERR_BAD_ARG;
    for (int k = 0; k < n; k++)
        if (!d_stack[k]) return UGSM_ERR_BAD_ARG;
    const int levels = ctx->cfg.levels, F = ctx->cfg.fovea_levels;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, levels, w, h));
    if (F < 2 || F > levels) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    FoveaGeom g[UGSM_MAX_BATCH];
    for (int k = 0; k < n; k++) fovea_geometry(w, h, F, off_x ? off_x[k] : 0, off_y ? off_y[k] : 0, g[k]);
    const size_t fl = (size_t)g[0].fw * g[0].fh;
    UCHK(ensure_level_bufs(ctx, *s, 3 * (size_t)w[1] * h[1]));
    // level F-1 (whole frame; the same in every stack) as a 3-plane field, from stack 0
    float *cur = s->d0, *other = s->d1;
    for (int c = 0; c < 3; c++)
        HIPCHK(ctx, hipMemcpyAsync(cur + c * fl, d_stack[0] + ((size_t)c * F + (F - 1)) * fl, fl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    for (int level = F - 1; level > 0; level--) {
        float *dst = (level == 1) ? d_out3 : other;
        PasteWindows pw{};
        pw.n = n;
        for (int k = 0; k < n; k++) {
            pw.org_x[k] = g[k].ox[level - 1];
            pw.org_y[k] = g[k].oy[level - 1];
            pw.stack[k] = byte_diff(d_stack[k], d_stack[0]);
        }
        Timer t(ctx, s, slot, KC_MISC, (double)w[level - 1] * h[level - 1]);
        launch_upsample_paste_multi(s->st, cur, w[level], h[level], dst, w[level - 1], h[level - 1], d_stack[0] + (size_t)(level - 1) * fl, (size_t)F * fl,
                                    g[0].fw, g[0].fh, pw);
        std::swap(cur, other);
    }
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

}  // extern "C"
