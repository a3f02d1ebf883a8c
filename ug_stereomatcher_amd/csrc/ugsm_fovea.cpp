// ugsm_fovea.cpp -- the foveated calls: the windows of a call's pairs, the fine phase (matching() with foveatedmatching == 1 below level
// F-1), the call with its LR check in lockstep, the warm call from a prior stack, several windows on one pair and their checked form, and
// hierarchicalDisparity over the stacks.  The coarse phase is the full-frame descent stopped at level F-1 (enqueue_fovea_coarse,
// ugsm_full.cpp); the levels' own work is ugsm_levels.cpp.  At the end the ugsm_submit_* entry points of the family.
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

// pair 0's range word into the entries 1 .. m - 1 (windows of one pair run under its word), doubling what is already there
int spread_range_word(ugsm_ctx *ctx, Slot &s, int m)
{
    for (int c = 1; s.range_known && c < m; c *= 2)
        HIPCHK(ctx, hipMemcpyAsync(s.range_bad + c, s.range_bad, sizeof(unsigned) * std::min(c, m - c), hipMemcpyDeviceToDevice, s.st));
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

// One foveated call of n pairs on device buffers: the pyramids, the coarse levels, the fine levels into the pairs' stacks.  state: n buffers
// of 3 fovW fovH floats for level F-1's field between the two phases; d_pyrL / d_pyrR as for enqueue_fovea_fine.
// With the foveated LR check on (ugsm_set_lr_check) the call matches both directions in lockstep and checks the stacks against each other:
//   - the pyramids are built once; entry n + b of the shape reads pair b's with the L and R views exchanged (pair_pyr), through pair b's windows
//     and seed maps, under pair b's range word (it covers both images' pyramids: build_pyramids reports either image into range_bad[pair]);
//     every kernel of a level takes the 2 n entries in one launch except K-cost, which takes each direction in one (run_level);
//   - every field of a foveated call is at most fovW x fovH, so the 2 n fields lie in the slot's level buffers at a stride of one such field
//     (n pairs hold n x 3 W H floats per buffer and need 2 n x 3 fovW fovH, fovW fovH <= W H / 2 for every F >= 2: it fits, for F = 2 just);
//   - what does NOT fit there for F = 2 is the right-to-left STACK, which has to outlive the fine levels: A, d0 and d1 are then full.  It goes,
//     with the right-to-left state, into the slot's LR buffer (Slot::lr, what the full-mode check keeps its second field in; lr_room): 3 (F + 1)
//     fovW fovH floats per pair, 24 MB at 16 MP beside the pair's 1.35 GB, counted by ugsm_context_device_bytes;
//   - one launch checks every level of every pair's stack after the last level (enqueue_lr_stack_check).
int enqueue_match_foveated(ugsm_ctx *ctx, Slot &s, int si, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                                 const int *off_x, const int *off_y, float *const *state, float *const *d_stack, float *const *d_pyrL, float *const *d_pyrR)
{
    const int F = ctx->cfg.fovea_levels;
    FoveaWin win;
    UCHK(fovea_windows(ctx, W, H, n, off_x, off_y, win));
    if (!lr_fovea_on(ctx)) {
        // (a single pair alone on the chip gets level F-1 .. top's A planes from the side stream; a batch computes A in line)
        UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, n, W, H, stride, n == 1 ? F - 1 : -1, &win));
        const Shape sh = Shape::pairs(s);
        UCHK(enqueue_fovea_coarse(ctx, s, si, sh, state));
        return enqueue_fovea_fine(ctx, s, si, sh, state, off_x, off_y, d_stack, d_pyrL, d_pyrR);
    }
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, n, W, H, stride, -1, &win));
    const int fw = s.w[F - 1], fh = s.h[F - 1];
    const Shape sh = Shape::both_directions(n, field_room((size_t)fw * fh));
    const LrRoom room = lr_room(n, F, fw, fh, false);
    UCHK(ensure_level_bufs(ctx, s, sh.nb * sh.stride));  // (holds already: see above)
    UCHK(grow(ctx, s.lr, s.lr_cap, room.total));
    UCHK(lr_host_ready(ctx, s));
    if (s.range_known) HIPCHK(ctx, hipMemcpyAsync(s.range_bad + n, s.range_bad, sizeof(unsigned) * n, hipMemcpyDeviceToDevice, s.st));
    float *vstate[2 * kMaxBatch], *vstack[2 * kMaxBatch];
    for (int b = 0; b < n; b++) {
        vstate[b] = state[b];
        vstack[b] = d_stack[b];
        vstack[n + b] = s.lr + (size_t)b * room.per;
        vstate[n + b] = vstack[n + b] + room.state;
    }
    UCHK(enqueue_fovea_coarse(ctx, s, si, sh, vstate));
    UCHK(enqueue_fovea_fine(ctx, s, si, sh, vstate, off_x, off_y, vstack, d_pyrL, d_pyrR));
    return enqueue_lr_stack_check(ctx, s, si, n, F, fw, fh, ctx->lr_tau, d_stack, room.per, reinterpret_cast<unsigned long long *>(s.lr + room.cnt));
}

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
    int turn = 0;
    if (table) {
        UCHK(grow(ctx, s.warm_tab, s.warm_tab_cap, (size_t)kMaxBatch));
        if (!s.warm_tab_h) HIPCHK(ctx, hipHostMalloc((void **)&s.warm_tab_h, Slot::kWarmRing * kMaxBatch * sizeof(RestrictStackRow), hipHostMallocDefault));
        turn = s.warm_next;
        s.warm_next = (turn + 1) % Slot::kWarmRing;
        if (!s.warm_ev[turn]) HIPCHK(ctx, hipEventCreateWithFlags(&s.warm_ev[turn], hipEventDisableTiming));
        if (s.warm_ev_set[turn]) HIPCHK(ctx, hipEventSynchronize(s.warm_ev[turn]));  // (the upload of the call kWarmRing back: long done)
        rows = s.warm_tab_h + (size_t)turn * kMaxBatch;
    }
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
        HIPCHK(ctx, hipMemcpyAsync(s.warm_tab, rows, (size_t)n * sizeof(RestrictStackRow), hipMemcpyHostToDevice, s.st));
        HIPCHK(ctx, hipEventRecord(s.warm_ev[turn], s.st));
        s.warm_ev_set[turn] = true;
        rs.table = s.warm_tab;
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

// The warm foveated call (ugsm_submit_foveated_warm[_field]; its refusals: ugsm_fovea_seeded.cpp): n pairs in lockstep from fovea level `start`
// of their priors.  The pyramids stop at level max(start, 2), level 0 inside the new windows; A is computed in line at every level (level F-1,
// where it is matched, included: the side stream's A planes serve the coarse phase, which does not run).  One launch writes every starting
// field: level `start`'s into the level buffer the fine phase starts in, the levels above into the stacks' row blocks.
int enqueue_match_foveated_warm(ugsm_ctx *ctx, Slot &s, int si, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                                const int *off_x, const int *off_y, const float *const *d_prior, const int *poff_x, const int *poff_y, bool field, int start,
                                float *const *d_stack)
{
    const int F = ctx->cfg.fovea_levels;
    FoveaWin win;
    UCHK(fovea_windows(ctx, W, H, n, off_x, off_y, win));
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, n, W, H, stride, -1, &win, false, 0, start));
    const Shape sh = Shape::pairs(s);
    UCHK(enqueue_restrict_stack(ctx, s, si, n, s.w, s.h, F, d_prior, poff_x, poff_y, field, off_x, off_y, start, d_stack, s.d0, sh.stride));
    return enqueue_fovea_fine(ctx, s, si, sh, nullptr, off_x, off_y, d_stack, nullptr, nullptr, start);
}
int fovea_warm_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride, const int *off_x,
                            const int *off_y, const float *const *d_prior, const int *prior_off_x, const int *prior_off_y, int field, int start_level,
                            float *const *d_stack)
{
    const int zeros[UGSM_MAX_BATCH] = {0};
    const int *ox = off_x ? off_x : zeros, *oy = off_y ? off_y : zeros, *px = prior_off_x ? prior_off_x : zeros, *py = prior_off_y ? prior_off_y : zeros;
    const int per = (n == 1 || fovea_batch_runs_pair_by_pair(ctx)) ? 1 : n;  // (kernel_path 1: the pairs one after the other, as ugsm_submit_foveated_batch)
    return submit_pairs(ctx, slot, n, per, [&](Slot &s, int b, int k) {
        return enqueue_match_foveated_warm(ctx, s, slot, k, d_rgbL + b, d_rgbR + b, W, H, stride, ox + b, oy + b, d_prior + b, px + b, py + b, field != 0,
                                           start_level, d_stack + b);
    });
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

// n fovea windows on ONE pair (ugsm_submit_foveated_multi): what does not depend on the window runs once, the rest in lockstep.
//   - the pyramids of one pair, as a lone foveated call builds them (side stream and A planes of levels F-1 .. top included), but with no
//     level 0 (FoveaWin::later); one launch then writes level 0 of both images inside the n windows (k_level0_windows).  Pyramids
//     that k_pyr_base does not build (fewer than three levels, kernel_path 1) hold level 0 whole and skip that launch;
//   - the coarse phase once, its field into `state`;
//   - the fine phase on a shape of n windows that all read pair 0's pyramids (Shape::one_pair, pair_pyr), start from the one state and
//     run under pair 0's range word; their fields lie in the level buffers at a stride of one fovea field, as a checked call's do.  The
//     caller has made the buffers hold n such fields (n x 3 fovW fovH floats exceed one pair's 3 W H as soon as n > 2^(F-1));
//   - contexts that run pair by pair (early exit, kernel_path 1) and n == 1: the fine phase window after window, as single pairs.
// Afterwards the slot holds no whole pyramids (have_pyr, have_coarse false).
int enqueue_foveated_multi(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int n,
                           const int *off_x, const int *off_y, float *state, float *const *d_stack)
{
    const int F = ctx->cfg.fovea_levels;
    FoveaWin win;
    UCHK(fovea_windows(ctx, W, H, n, off_x, off_y, win));
    win.later = true;
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, W, H, stride, F - 1, &win));
    UCHK(enqueue_level0_windows(ctx, s, si, d_rgbL, d_rgbR, stride, n, win));
    int st = enqueue_fovea_coarse(ctx, s, si, state);
    if (st == UGSM_OK) {
        if (n == 1 || ctx->cfg.kernel_path == 1 || ctx->cfg.early_exit_threshold > 0.0f) {
            for (int k = 0; k < n && st == UGSM_OK; k++) st = enqueue_fovea_fine(ctx, s, si, state, off_x[k], off_y[k], d_stack[k], nullptr, nullptr);
        } else {
            const Shape sh = Shape::windows(n, field_room((size_t)win.w * win.h));
            if (sh.nb * sh.stride > s.lvl_cap) {
                ctx->err = "the level buffers do not hold the windows' fields";
                return UGSM_ERR_STATE;
            }
            UCHK(spread_range_word(ctx, s, n));
            const float *vstate[kMaxBatch];
            for (int k = 0; k < n; k++) vstate[k] = state;
            st = enqueue_fovea_fine(ctx, s, si, sh, vstate, off_x, off_y, d_stack, nullptr, nullptr);
        }
    }
    s.have_pyr = false;
    s.have_coarse = false;
    return st;
}

// ugsm_submit_foveated_multi_checked: n windows of one pair, both directions in lockstep, the n stacks checked against their right-to-left twins.
// enqueue_foveated_multi and the checked enqueue_match_foveated composed:
//   - one pair's pyramids with no level 0 and the one k_level0_windows launch, as the plain multi call (no A planes from the side stream: the
//     coarse phase runs on two entries and computes A in line, as every batch does).  The right-to-left direction reads the same two
//     pyramids, so nothing more is stored;
//   - pair 0's range word into the entries 1 .. 2 n - 1;
//   - the coarse phase once for the two directions (Shape::coarse_both_directions: entry 1 = pair 0 exchanged, pair_pyr), level F-1's two
//     fields into `state` and into the LR buffer;
//   - the fine phase on Shape::windows_both_directions: entry k is window k left-to-right from the first state, entry n + k window k
//     right-to-left from the second, its stack in the LR buffer.  K-cost runs one launch per direction and level (cost_groups); more than
//     kMaxBatch entries go through launches of equal size (group_pairs);
//   - one launch of k_lr_check's stack form over the n (window, level) entries with the call's own tau (enqueue_lr_stack_check).
// The caller has made the level buffers hold 2 n fovea fields and the LR buffer lr_room(.., true).total floats.
int enqueue_foveated_multi_checked(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int n,
                                   const int *off_x, const int *off_y, float *state, float *const *d_stack, float tau)
{
    const int F = ctx->cfg.fovea_levels;
    FoveaWin win;
    UCHK(fovea_windows(ctx, W, H, n, off_x, off_y, win));
    win.later = true;
    UCHK(enqueue_pyramids(ctx, s, si, d_rgbL, d_rgbR, W, H, stride, -1, &win));
    UCHK(enqueue_level0_windows(ctx, s, si, d_rgbL, d_rgbR, stride, n, win));
    const size_t field = field_room((size_t)win.w * win.h);
    const Shape sh = Shape::windows_both_directions(n, field);
    const LrRoom room = lr_room(n, F, win.w, win.h, true);
    if (sh.nb * sh.stride > s.lvl_cap || room.total > s.lr_cap || !s.lr_host) {
        ctx->err = "the slot's buffers do not hold the checked windows' fields";
        return UGSM_ERR_STATE;
    }
    UCHK(spread_range_word(ctx, s, 2 * n));
    float *vstate[2 * kMaxBatch], *vstack[2 * kMaxBatch];
    for (int k = 0; k < n; k++) {
        vstate[k] = state;
        vstate[n + k] = s.lr + room.state;
        vstack[k] = d_stack[k];
        vstack[n + k] = s.lr + (size_t)k * room.per;
    }
    float *const cstate[2] = {state, s.lr + room.state};
    s.have_pyr = false;
    UCHK(enqueue_fovea_coarse(ctx, s, si, Shape::coarse_both_directions(field), cstate));
    UCHK(enqueue_fovea_fine(ctx, s, si, sh, vstate, off_x, off_y, vstack, nullptr, nullptr));
    return enqueue_lr_stack_check(ctx, s, si, n, F, win.w, win.h, tau, d_stack, room.per, reinterpret_cast<unsigned long long *>(s.lr + room.cnt));
}

// ---- n windows on one pair ----------------------------------------------------------------------------------------------------
// What ugsm_submit_foveated_multi and ugsm_match_foveated_multi refuse before anything is enqueued; the windows' field size on success.
// tau: null = the plain call; else the checked call's threshold (ugsm_submit_foveated_multi_checked), which has refusals of its own and does
// not look at the context's setting.
int multi_check(ugsm_ctx *ctx, int n, int W, int H, int stride, const int *&off_x, const int *&off_y, const int *zeros, int *fw, int *fh,
                const float *tau)
{
    const int F = ctx->cfg.fovea_levels;
    if (n < 1 || n > UGSM_MAX_BATCH || F < 2) return UGSM_ERR_BAD_ARG;
    if (!off_x) off_x = zeros;
    if (!off_y) off_y = zeros;
    if (tau && !(*tau > 0.0f)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked multi-window call needs tau > 0");
    // (ugsm_set_lr_check's rule: these contexts run every level pair by pair and have no batch dimension to carry the second direction in)
    if (tau && (ctx->cfg.early_exit_threshold > 0.0f || ctx->cfg.kernel_path == 1))
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the checked multi-window call: not with early_exit_threshold > 0 or kernel_path 1");
    if (!tau && lr_fovea_on(ctx)) return ctx_fail(ctx, UGSM_ERR_STATE, "the foveated LR check is on: the checked multi-window call is ugsm_submit_foveated_multi_checked (ugsm_set_lr_check)");
    UCHK(ugsm_fovea_dims(W, H, ctx->cfg.levels, F, fw, fh));
    UCHK(input_status(ctx, W, stride));
    return UGSM_OK;
}
// the level buffers for n fields of fw x fh in lockstep (contexts that run window by window need one pair's alone)
int multi_level_bufs(ugsm_ctx *ctx, Slot &s, int n, int W, int H, int fw, int fh)
{
    if (n == 1 || ctx->cfg.kernel_path == 1 || ctx->cfg.early_exit_threshold > 0.0f) return UGSM_OK;
    return ensure_level_bufs(ctx, s, std::max((size_t)n * field_room((size_t)fw * fh), 3 * (size_t)W * H));
}

// ... and of the checked call: 2 n fields in the level buffers, the right-to-left stacks, state and count words in the LR buffer
int multi_checked_bufs(ugsm_ctx *ctx, Slot &s, int n, int W, int H, int fw, int fh)
{
    UCHK(ensure_level_bufs(ctx, s, std::max(2 * (size_t)n * field_room((size_t)fw * fh), 3 * (size_t)W * H)));
    UCHK(grow(ctx, s.lr, s.lr_cap, lr_room(n, ctx->cfg.fovea_levels, fw, fh, true).total));
    return lr_host_ready(ctx, s);
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
    const int F = ctx->cfg.fovea_levels;
    if (F < 2) return UGSM_ERR_BAD_ARG;
    // level F-1's state is staged in the slot's hout
    int fw, fh;
    UCHK(ugsm_fovea_dims(W, H, ctx->cfg.levels, F, &fw, &fh));
    const size_t fn3 = 3 * (size_t)fw * fh;
    UCHK(grow(ctx, s->hout, s->hout_cap, std::max(fn3, s->hout_cap)));
    UCHK(enqueue_match_foveated(ctx, *s, slot, 1, &d_rgbL, &d_rgbR, W, H, stride, &off_x, &off_y, &s->hout, &d_stack, d_pyrL ? &d_pyrL : nullptr,
                          d_pyrR ? &d_pyrR : nullptr));
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
    const int F = ctx->cfg.fovea_levels;
    if (F < 2) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    int zeros[UGSM_MAX_BATCH] = {0};
    const int *ox = off_x ? off_x : zeros, *oy = off_y ? off_y : zeros;
    int fw, fh;
    UCHK(ugsm_fovea_dims(W, H, ctx->cfg.levels, F, &fw, &fh));
    const size_t fn3 = field_room((size_t)fw * fh);  // level F-1's state of every pair, staged in the slot's hout
    UCHK(grow(ctx, s->hout, s->hout_cap, std::max(fn3 * n, s->hout_cap)));
    if (n == 1 || fovea_batch_runs_pair_by_pair(ctx)) {
        for (int b = 0; b < n; b++)
            UCHK(enqueue_match_foveated(ctx, *s, slot, 1, d_rgbL + b, d_rgbR + b, W, H, stride, ox + b, oy + b, &s->hout, d_stack + b,
                                  (d_pyrL && d_pyrL[b]) ? d_pyrL + b : nullptr, (d_pyrR && d_pyrR[b]) ? d_pyrR + b : nullptr));
        return mark_done(ctx, *s);
    }
    float *state[UGSM_MAX_BATCH];
    for (int b = 0; b < n; b++) state[b] = s->hout + b * fn3;
    UCHK(enqueue_match_foveated(ctx, *s, slot, n, d_rgbL, d_rgbR, W, H, stride, ox, oy, state, d_stack, d_pyrL, d_pyrR));
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
    const int zeros[UGSM_MAX_BATCH] = {0};
    int fw, fh;
    UCHK(multi_check(ctx, n, W, H, stride, off_x, off_y, zeros, &fw, &fh, tau));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(tau ? multi_checked_bufs(ctx, *s, n, W, H, fw, fh) : multi_level_bufs(ctx, *s, n, W, H, fw, fh));
    const size_t fn3 = 3 * (size_t)fw * fh;  // the (left-to-right) level-F-1 state, staged in the slot's hout as ugsm_submit_foveated stages it
    UCHK(grow(ctx, s->hout, s->hout_cap, std::max(fn3, s->hout_cap)));
    if (tau) UCHK(enqueue_foveated_multi_checked(ctx, *s, slot, d_rgbL, d_rgbR, W, H, stride, n, off_x, off_y, s->hout, d_stack, *tau));
    else UCHK(enqueue_foveated_multi(ctx, *s, slot, d_rgbL, d_rgbR, W, H, stride, n, off_x, off_y, s->hout, d_stack));
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
