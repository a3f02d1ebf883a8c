// ugsm_levels.cpp -- the work of one level, for every call's sequence (ugsm_full.cpp, ugsm_fovea.cpp) and the stage-level entry points
// (ugsm_stages.cpp): the pyramids, A = G_clamp * L^2, the iterations of K-cost and K-smooth (run_level), the seed hand-over between levels.
// Which kernel a launch runs is asked of ugsm_policy.cpp; the vocabulary -- Grp, Shape, for_groups, FoveaWin -- is in ugsm_slot.hpp.
#include "ugsm_device.hpp"
#include "ugsm_slot.hpp"

#include <algorithm>

using namespace ugsm;

namespace ugsm {
namespace {
// The Batch argument of a group's launch.  Inputs and outputs are the slot's level buffers (entry b at + b * sh.stride) unless
// `outs` names per-pair destinations (the callers' buffers); `views`: the L / R views of the pairs (fovea windows sit at different
// places); `seeds`: their seed-crop origins.  All arrays are indexed by the pair's number in the batch.
Batch make_batch(const Shape &sh, Grp g, const Img3 *views = nullptr, const SeedMap *seeds = nullptr, float *const *outs = nullptr)
{
    Batch b{};
    b.n = g.n;
    for (int j = 0; j < g.n; j++) {
        b.in[j] = (long long)(j * sh.stride * sizeof(float));
        b.out[j] = outs ? byte_diff(outs[g.b0 + j], outs[g.b0]) : b.in[j];
        b.img[j] = views ? byte_diff(views[g.b0 + j].p, views[g.b0].p) : 0;
        b.cx[j] = seeds ? seeds[g.b0 + j].cx : 0;
        b.cy[j] = seeds ? seeds[g.b0 + j].cy : 0;
    }
    return b;
}

}  // namespace

// a batched plane copy: entry j of group g from src0 + j * sh.stride (a level buffer) or from its view, to its own destination
Batch copy_batch(const Shape &sh, Grp g, const Img3 *views, float *const *dsts, size_t dst_off)
{
    Batch b{};
    b.n = g.n;
    for (int j = 0; j < g.n; j++) {
        b.img[j] = views ? byte_diff(views[g.b0 + j].p, views[g.b0].p) : (long long)(j * sh.stride * sizeof(float));
        b.out[j] = byte_diff(dsts[g.b0 + j] + dst_off, dsts[g.b0] + dst_off);
    }
    return b;
}

// CreatePyramidFromImage (MatchGPULib.cpp:1033-1125) for the left OR the right image of every pair of the call: rgb[b] -> pyr + b * pyr_stride.
// The images of a batch go through every pyramid kernel together (one launch per level for all of them).
// skip0 (full-mode calls whose level-0 kernels read the images: Slot::direct0): level 0 is not stored at all.
// built (a seeded call, which matches no level above its first): only the levels 0 .. built - 1 are produced; 0: all of them.
int build_pyramids(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *const *rgb, int stride, float *pyr, hipStream_t stream, const FoveaWin *win, bool skip0, int built)
{
    const hipStream_t pst = stream ? stream : s.st;  // (launches on the side stream are not bracketed by events: Timer records on s.st)
    const int levels = (built > 0 && built < s.levels) ? built : s.levels, nb = s.nb;
    const bool ref = ctx->cfg.kernel_path == 1;
    // levels 0, 1, 2 in one pass over the rgb8 input (k_pyr_base); the one-stage-per-kernel path keeps the three launches
    const bool base = !ref && levels >= 3;
    Batch bt{};  // image j of the launch = pair j: its rgb8 input, its pyramid, its range word
    bt.n = nb;
    for (int j = 0; j < nb; j++) {
        bt.img[j] = byte_diff(rgb[j], rgb[0]);
        bt.in[j] = bt.out[j] = (long long)(j * s.pyr_stride * sizeof(float));
        bt.cx[j] = j;
    }
    Batch bt0 = bt;  // k_pyr_base: the input-field offsets carry the pairs' window origins instead
    if (win || skip0)
        for (int j = 0; j < nb; j++) bt0.in[j] = win ? ((long long)win->y0[j] << 32) | (unsigned)win->x0[j] : 0;
    const bool later = win && win->later;
    const PyrWindow pw = later ? kPyrNoLevel0 : (win ? PyrWindow{win->x0[0], win->y0[0], win->w, win->h} : (skip0 ? kPyrNoLevel0 : PyrWindow{0, 0, 0, 0}));
    if ((skip0 && (win || !base)) || (later && nb != 1)) {  // (level0_direct asks for neither; the windows of ONE pair come later)
        ctx->err = "pyramids without level 0 are built by k_pyr_base for full-mode calls, and for the one pair of a multi-window call";
        return UGSM_ERR_STATE;
    }
    const Batch *const pb = nb > 1 ? &bt : nullptr;
    const long long stream_min = pyramid_stream_min(s, win != nullptr);
    s.cur_level = 0;
    if (base) {
        Timer t(ctx, &s, si, KC_PYR_BASE, (double)s.W * s.H * nb);
        launch_pyr_base(pst, rgb[0], stride, s.W, s.H, pyr + s.off[0], pyr + s.off[1], s.w[1], s.h[1], pyr + s.off[2], s.w[2], s.h[2], s.range_bad,
                        nb > 1 ? &bt0 : nullptr, pw, ctx->hooks.input_format);
    } else {
        // (pyramids of fewer than three levels, and kernel_path 1: image by image)
        for (int b = 0; b < nb; b++) {
            Timer t(ctx, &s, si, KC_MISC, (double)s.W * s.H);
            launch_rgb_planes(pst, rgb[b], stride, s.W, s.H, pyr + b * s.pyr_stride + s.off[0], ctx->hooks.input_format);
            // (a float level 0 is the caller's: k_pyr_base checks it as it reads it, this path once it is written)
            if (input_float(ctx->hooks.input_format) && s.range_known)
                launch_range_scan(pst, pyr + b * s.pyr_stride + s.off[0], 3 * (size_t)s.W * s.H, s.range_bad + b);
        }
    }
    // CreatePyramidFromImage, MatchGPULib.cpp:1063-1106: level 1 from level 0 (sf=(float)SCALE),
    // level i+2 from level i (sf=2.0f).  Levels are produced in dependency order.
    for (int i = 0; i < levels; i++) {
        if (i == 0 && levels > 1 && !base) {
            s.cur_level = 1;
            Timer t(ctx, &s, si, KC_PYR, (double)s.w[1] * s.h[1] * nb);
            float sf = (float)kScale;
            if (ref) launch_blur_decimate_ref(pst, pyr + s.off[0], s.w[0], s.h[0], pyr + s.off[1], s.w[1], s.h[1], sf);
            else launch_blur_decimate(pst, pyr + s.off[0], s.w[0], s.h[0], pyr + s.off[1], s.w[1], s.h[1], sf, s.range_bad, pb, stream_min);
        }
        if (i + 2 < levels && !(base && i == 0)) {
            s.cur_level = i + 2;
            Timer t(ctx, &s, si, KC_PYR, (double)s.w[i + 2] * s.h[i + 2] * nb);
            float sf = (float)(0.000 + (int)(kScale * kScale + 0.5));  // :1090
            if (ref) launch_blur_decimate_ref(pst, pyr + s.off[i], s.w[i], s.h[i], pyr + s.off[i + 2], s.w[i + 2], s.h[i + 2], sf);
            else launch_blur_decimate(pst, pyr + s.off[i], s.w[i], s.h[i], pyr + s.off[i + 2], s.w[i + 2], s.h[i + 2], sf, s.range_bad, pb, stream_min);
        }
    }
    s.cur_level = kNoLevel;
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

// S Jacobi passes + the 3x3 box (MatchGPULib.cpp:2257-2412) for every entry of the call.  On return `a` holds the
// result and `b` is scratch (base pointers: entry k's buffers lie at + k * sh.stride).
// final_out (optional, fused path): per-pair destinations; the last launch writes there instead of into `b`, and `a` is then not meaningful.
int enqueue_smooth(ugsm_ctx *ctx, Slot &s, int si, const Shape &sh, float *&a, float *&b, int W, int H, int S, bool do_box, float *const *final_out)
{
    const double px = (double)W * H;
    if (ctx->cfg.kernel_path == 1) {  // (never batched)
        for (int j = 0; j < S; j++) {
            Timer t(ctx, &s, si, KC_SMOOTH, px);
            launch_smooth_pass_ref(s.st, a, b, W, H);
            std::swap(a, b);
        }
        if (do_box) {
            Timer t(ctx, &s, si, KC_BOX, px);
            launch_box_ref(s.st, a, b, W, H);
            std::swap(a, b);
        }
    } else {
        const int pairs = launch_pairs(ctx, sh, W, H);
        int left = S;
        do {
            int p = std::min(left, 5);
            left -= p;
            if (p == 0 && !do_box) break;
            const int rh = (ctx->small_mask & 2) ? small_rh(ctx, W, H, s.alone, pairs) : 0;
            const bool box_now = do_box && left == 0;
            const bool to_final = left == 0 && final_out;
            for_groups(sh.nb, pairs > 1, [&](Grp g) {
                Timer t(ctx, &s, si, rh ? KC_SMOOTH_SMALL : KC_SMOOTH, px * g.n);
                const float *src = a + g.b0 * sh.stride;
                float *dst = to_final ? final_out[g.b0] : b + g.b0 * sh.stride;
                const Batch bt = make_batch(sh, g, nullptr, nullptr, to_final ? final_out : nullptr);
                const Batch *pb = g.n > 1 ? &bt : nullptr;
                if (rh) launch_smooth_small(s.st, src, dst, W, H, p, box_now, rh, pb);
                else launch_smooth_fused(s.st, src, dst, W, H, p, box_now, smooth_rows_for(ctx, W, H, s.alone, g.n), pb, smooth_class_for(W, H, g.n));
            });
            if (!to_final) std::swap(a, b);
        } while (left > 0);
    }
    return UGSM_OK;
}

// Row f-4 (MatchGPULib.cpp:1323-1437): S_dx / C and S_dy / C of two device fields, synchronously (one host round trip).
int weighted_difference(ugsm_ctx *ctx, Slot &s, const float *newd3, const float *oldd3, int W, int H, float out2[2])
{
    const size_t need = 3 * (size_t)H + 3;
    UCHK(s.wd_rows.grow(ctx, need));
    UCHK(s.wd_host.grow(ctx, 3));
    double *tot = s.wd_rows + 3 * (size_t)H;
    launch_weighted_difference(s.st, newd3, oldd3, W, H, s.wd_rows, tot);
    HIPCHK(ctx, hipMemcpyAsync(s.wd_host, tot, 3 * sizeof(double), hipMemcpyDeviceToHost, s.st));
    HIPCHK(ctx, hipStreamSynchronize(s.st));
    out2[0] = (float)(s.wd_host[0] / s.wd_host[2]);
    out2[1] = (float)(s.wd_host[1] / s.wd_host[2]);
    return UGSM_OK;
}

// matchlevel (MatchGPULib.cpp:1662-2489), iterations m_from..m_to, for every entry of the call (sh.nb; in lockstep).  Lv / Rv: the entries'
// views of the level (sh.nb of them).  cur holds (dx,dy,conf) on entry and on exit; other is scratch of the same size (base pointers:
// entry k's fields lie at + k * sh.stride).
// final_out (optional, fused path only): per-pair destinations where the last iteration leaves its result instead of the ping-pong buffer
// (saves the device-to-device copy of the finished level); cur/other are then not meaningful afterwards.
// seed (optional, see fuse_seed; sh.nb entries): `cur` holds the COARSER level's field (seed->Ws x seed->Hs) and iteration m_from reads its
// starting field through the seeding map instead of from a materialised seeded field.
// A_pre (optional, single pairs only): A = G_clamp * L^2 of this level, already computed (on the slot's side stream; the caller has made
// the main stream wait for it); otherwise it is computed here, into s.A.
// in (kInPlanes, or kInRGB8: level 0 of a call with Slot::direct0): Lv / Rv are byte views of the pairs' images; the level runs k_cost_march
// (level0_direct has seen to it) and any seed map has its origin at 0.  A shape of both directions may bring them too: a K-cost launch holds
// the entries of one direction (cost_groups), so one R offset per entry serves it, and A = G * L^2 reads the L view alone.
int run_level(ugsm_ctx *ctx, Slot &s, int si, const Shape &sh, const Img3 *Lv, const Img3 *Rv, int W, int H, int mi, int S, bool is_top, int m_from,
              int m_to, float *&cur, float *&other, float *dbg8, float *const *final_out, const SeedMap *seed, const float *A_pre, int in)
{
    const bool ref = ctx->cfg.kernel_path == 1;
    const double px = (double)W * H;
    std::vector<float> thr((size_t)std::max(mi, 1));
    threshold_schedule(mi, thr.data());
    // row f-4, opt-in: stop the level when the confidence-weighted mean change of dx and dy falls below the threshold.  The
    // previous iteration's field has to survive the smoothing ping-pong, hence a third buffer.
    const float eps = ctx->cfg.early_exit_threshold;
    const bool early = eps > 0.0f;
    if ((early || ref) && sh.nb != 1) return UGSM_ERR_STATE;  // (the batch entry points run such contexts pair by pair)
    float *third = nullptr;
    if (early) {
        const size_t lvl = 3 * (size_t)W * H;
        UCHK(s.d2.grow(ctx, std::max<size_t>(lvl, s.lvl_cap)));
        // the three field buffers rotate through the levels: the spare one is whichever is neither `cur` nor `other` right now
        third = (s.d0 != cur && s.d0 != other) ? s.d0 : ((s.d1 != cur && s.d1 != other) ? s.d1 : s.d2);
        final_out = nullptr;
    }
    int ran = 0;
    const int pairs = launch_pairs(ctx, sh, W, H);
    const bool batched = pairs > 1;
    const bool march4 = !ref && use_march4(ctx, W, H, s.alone, pairs);
    const bool march = !ref && use_march(ctx, W, H, s.alone, pairs);
    const bool small = !ref && use_small_cost(ctx, W, H, s.alone, pairs);
    if (in != kInPlanes) {  // byte views: what level0_direct promised must hold here, and the seed-crop origins -- whose Batch fields carry the R offsets -- are 0
        bool origins0 = true;
        for (int b = 0; seed && b < sh.nb; b++) origins0 = origins0 && seed[b].cx == 0 && seed[b].cy == 0;
        if (in != kInRGB8 || march4 || !march || early || !origins0) {
            ctx->err = in != kInRGB8 ? "level 0 from the image: no kernel instance for this input form"
                       : !origins0   ? "level 0 from the image: a seed map with a crop origin (the rgb8 K-cost instance serves full mode only)"
                                     : "level 0 from the image needs the level matched by k_cost_march (kernel-choice policy: march_min_pixels, k_cost_march4's range) "
                                       "and no early exit";
            return UGSM_ERR_STATE;
        }
    }
    if (!ref && !march4 && !march && !small && !kDevLib) {  // (use_march gives every such level to k_cost_march: launch_cost_fused is a no-op here)
        ctx->err = "no K-cost kernel of libugsm.so covers this level (kernel-choice policy)";
        return UGSM_ERR_STATE;
    }
    const float *const A3 = A_pre ? A_pre : s.A;  // (entry k's A at + k * sh.stride)
    if (!A_pre) {   // A = G_clamp * L^2 does not depend on the iteration: once per level.
        for_groups(sh.nb, batched, [&](Grp g) {
            Timer t(ctx, &s, si, KC_SQBLUR, px * g.n);
            if (ref) {
                launch_sqblur_clamp_ref(s.st, Lv[g.b0], W, H, s.A);
            } else {
                const Batch bt = make_batch(sh, g, Lv);
                launch_sqblur_clamp(s.st, Lv[g.b0], W, H, s.A + g.b0 * sh.stride, g.n > 1 ? &bt : nullptr, in);
            }
        });
    }
    // (k_cost_split -- libugsm_dev.so, march_min_pixels < 0: the levels no other form covers -- has no batch index: pair by pair)
    const bool cost_batched = batched && (march4 || march || small);
    // K-cost moves an entry's L and R views by ONE offset (Batch::img), which serves the entries of one direction only -- entry b's views lie
    // b pyramids behind entry 0's in both images, entry nreal + b's do so with the images exchanged -- so where a shape holds both
    // directions (nreal < nb), a K-cost launch holds the entries of one: two launches where every other kernel of the level has one.
    auto cost_groups = [&](auto &&f) {
        if (sh.nb == sh.nreal) return for_groups(sh.nb, cost_batched, f);
        for (int dir = 0; dir < 2; dir++) for_groups(sh.nreal, cost_batched, [&](Grp g) { f(Grp{g.b0 + dir * sh.nreal, g.n}); });
    };
    for (int m = m_from; m <= m_to; m++) {
        const int blend = !(is_top && m == 1);  // MatchGPULib.cpp:2223
        if (ref) {
            {
                Timer t(ctx, &s, si, KC_WARP, px);
                launch_warp_ref(s.st, Rv[0], cur, W, H, s.Rw);
            }
            {
                Timer t(ctx, &s, si, KC_SQBLUR, px);
                launch_sqblur_clamp_ref(s.st, Img3{s.Rw, W, (size_t)W * H}, W, H, s.B);
            }
            Timer t(ctx, &s, si, KC_COST, px);
            launch_cost_ref(s.st, Lv[0], s.Rw, A3, s.B, cur, other, W, H, thr[m - 1], blend, (m == m_to) ? dbg8 : nullptr);
        } else {
            const bool seeded = seed && m == m_from;
            cost_groups([&](Grp g) {
                Timer t(ctx, &s, si, march4 ? KC_COST_MARCH4 : (march ? KC_COST_MARCH : (small ? KC_COST_SMALL : KC_COST)), px * g.n);
                const size_t fo = g.b0 * sh.stride;
                const Img3 L = Lv[g.b0], R = Rv[g.b0];
                Batch bt = make_batch(sh, g, Lv, seeded ? seed : nullptr);
                if (in != kInPlanes)  // (byte views: the R image of a pair has an offset of its own, carried where the seed-crop origins -- 0 here -- ride)
                    for (int j = 0; j < g.n; j++) {
                        const long long d = byte_diff(Rv[g.b0 + j].p, Rv[g.b0].p);
                        bt.cx[j] = (int)(unsigned)(d & 0xffffffffll);
                        bt.cy[j] = (int)(d >> 32);
                    }
                const Batch *pb = g.n > 1 ? &bt : nullptr;
                const unsigned *rb = s.range_known ? s.range_bad + g.b0 : nullptr;
                if (march4)
                    launch_cost_march4(s.st, L, R, A3 + fo, cur + fo, other + fo, W, H, thr[m - 1], blend, 0, rb, seeded ? seed[g.b0] : SeedMap{0, 0, 0, 0}, pb);
                else if (march && seeded)
                    launch_cost_march_seeded(s.st, L, R, A3 + fo, cur + fo, seed[g.b0], other + fo, W, H, thr[m - 1], blend, march_rows_arg(ctx), rb, pb, in);
                else if (march) launch_cost_march(s.st, L, R, A3 + fo, cur + fo, other + fo, W, H, thr[m - 1], blend, march_rows_arg(ctx), rb, pb, in);
                else if (small) launch_cost_small(s.st, L, R, A3 + fo, cur + fo, other + fo, W, H, thr[m - 1], blend, pb);
                else launch_cost_fused(s.st, L, R, A3 + fo, cur + fo, other + fo, W, H, thr[m - 1], blend);
            });
        }
        ran = m;
        if (early) {
            float *a = other, *b = third;  // cur (the field before this iteration) stays untouched
            UCHK(enqueue_smooth(ctx, s, si, sh, a, b, W, H, S, true, nullptr));
            float dif[2] = {0.0f, 0.0f};
            if (m < m_to) UCHK(weighted_difference(ctx, s, a, cur, W, H, dif));
            float *old = cur;
            cur = a;  // the new field; b and the old field are the scratch pair of the next iteration
            other = b;
            third = old;
            if (m < m_to && dif[0] < eps && dif[1] < eps) break;  // differenceIterations: both below the threshold
            continue;
        }
        float *a = other, *b = cur;
        UCHK(enqueue_smooth(ctx, s, si, sh, a, b, W, H, S, true, (m == m_to && !ref) ? final_out : nullptr));
        if (m == m_to && !ref && final_out) break;
        cur = a;
        other = b;
    }
    s.iters_run[s.cur_level == kNoLevel ? 0 : s.cur_level] = ran;
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

Img3 level_view(const Slot &s, const float *pyr, int lev, int ox, int oy)
{
    return Img3{pyr + s.off[lev] + (size_t)oy * s.w[lev] + ox, s.w[lev], (size_t)s.w[lev] * s.h[lev]};
}

// The pyramid that entry v of the call matches as its left (side 0) or right (side 1) image.  The entries nreal .. nb - 1 of a shape that
// holds both directions are the entries 0 .. nreal - 1 with the two exchanged: the right-to-left match reads the same two pyramids.  The
// entries of a multi-window call (Shape::one_pair) are windows of pair 0: every one reads its pyramids as they are -- and, in the checked
// multi-window call, the entries nreal .. nb - 1 read them with the two exchanged.
const float *pair_pyr(const Slot &s, const Shape &sh, int side, int v)
{
    const bool back = v >= sh.nreal;
    if (sh.one_pair) return (side == 0) != back ? s.pyrL : s.pyrR;  // (n windows of one pair: ugsm_submit_foveated_multi[_checked])
    return ((side == 0) != back ? s.pyrL : s.pyrR) + (size_t)(back ? v - sh.nreal : v) * s.pyr_stride;
}

// A = G_clamp * L^2 of the full-frame levels a_from .. top on the side stream, beside whatever the main stream does next (the right
// pyramid's join, the coarse levels' iterations); run_level takes them through level_A, which makes the main stream wait for each.
// a_top (a seeded call): the first level that is matched, where it is not the top one; < 0: the top level.
int enqueue_side_A(ugsm_ctx *ctx, Slot &s, int a_from, int a_top)
{
    if (a_from < 0 || ctx->cfg.early_exit_threshold > 0.0f) return UGSM_OK;
    size_t tot = s.off[s.levels - 1] + 3 * (size_t)s.w[s.levels - 1] * s.h[s.levels - 1];
    UCHK(s.Apyr.grow(ctx, tot));
    HIPCHK(ctx, hipEventRecord(s.ev_L, s.st));  // (the left pyramid is complete on the main stream)
    s.forked = true;
    HIPCHK(ctx, hipStreamWaitEvent(s.st2, s.ev_L, 0));
    for (int i = a_top >= 0 ? a_top : s.levels - 1; i >= a_from; i--) {  // coarsest first: that is the order the levels need them in
        if (i == 0 && s.direct0) launch_sqblur_clamp(s.st2, byte_view(s.img0L[0], s.img0_stride), s.w[0], s.h[0], s.Apyr + s.off[0], nullptr, kInRGB8);
        else launch_sqblur_clamp(s.st2, level_view(s, s.pyrL, i, 0, 0), s.w[i], s.h[i], s.Apyr + s.off[i]);
        HIPCHK(ctx, hipEventRecord(s.ev_A[i], s.st2));
    }
    s.a_from = a_from;
    return UGSM_OK;
}

// The pyramids of every pair of the call (s.nb = nb pairs; rgbL / rgbR: nb device pointers).
// a_from: the levels a_from .. top get their A = G_clamp * L^2 precomputed on the side stream (full mode: 0; foveated: F-1, the
// fine levels work on crops whose A is clamped at the crop's own border and is computed in line); < 0: none.
// full: the call is a full-mode match and nothing else reads these pyramids -- level 0 is then read from the images where level0_direct allows.
// entries: the fields the call's levels run in lockstep where that is not nb (level0_direct).
// first (a seeded call; < 0: none): the call matches the levels first .. 0 only: the pyramids hold the levels 0 .. max(first, 2) -- what k_pyr_base
// makes in its one pass, and the levels up to the first -- so nothing that needs whole pyramids may follow (have_pyr), and A stops at `first`.
int enqueue_pyramids(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int nb, int W, int H, int stride, int a_from,
                     const FoveaWin *win, bool full, int entries, int first)
{
    const int built = first < 0 ? 0 : std::max(first, 2) + 1;
    if (!d_rgbL || !d_rgbR || nb < 1 || nb > kMaxBatch) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < nb; b++)
        if (!d_rgbL[b] || !d_rgbR[b]) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < nb; b++) UCHK(input_status(ctx, W, stride, d_rgbL[b], d_rgbR[b]));
    UCHK(prepare_slot(ctx, s, W, H, nb));
    // the pyramid kernels of the fused path check every value they write (level 0 holds the integers 0..255)
    s.range_known = ctx->cfg.kernel_path != 1 && s.range_bad != nullptr;
    if (s.range_known) HIPCHK(ctx, hipMemsetAsync(s.range_bad, 0, sizeof(unsigned) * nb, s.st));
    // One stream, as in rounds 1 and 2: the one-stage-per-kernel path, a batch, and whenever launches are bracketed by events (the
    // statistics belong to one stream).  Otherwise fork: R's pyramid and the A planes on the side stream.
    const bool fork = side_stream_ok(ctx, s);
    s.a_from = -1;
    const bool direct0 = full && !win && level0_direct(ctx, s, entries);
    s.direct0 = direct0;
    if (direct0) {
        for (int b = 0; b < nb; b++) {
            s.img0L[b] = d_rgbL[b];
            s.img0R[b] = d_rgbR[b];
        }
        s.img0_stride = stride;
    }
    if (!fork) {
        UCHK(build_pyramids(ctx, s, si, d_rgbL, stride, s.pyrL, nullptr, win, direct0, built));
        UCHK(build_pyramids(ctx, s, si, d_rgbR, stride, s.pyrR, nullptr, win, direct0, built));
        s.have_pyr = nb == 1 && !win && !direct0 && built == 0;  // (the fovea-shard entry points work on single pairs, and on whole pyramids)
        return UGSM_OK;
    }
    // the side stream starts after everything enqueued on this slot so far (the previous pair still reads pyrR and Apyr)
    HIPCHK(ctx, hipEventRecord(s.ev_in, s.st));
    s.forked = true;
    HIPCHK(ctx, hipStreamWaitEvent(s.st2, s.ev_in, 0));
    UCHK(build_pyramids(ctx, s, si, d_rgbR, stride, s.pyrR, s.st2, win, direct0, built));
    HIPCHK(ctx, hipEventRecord(s.ev_R, s.st2));
    UCHK(build_pyramids(ctx, s, si, d_rgbL, stride, s.pyrL, nullptr, win, direct0, built));
    if (a_from >= 0) UCHK(enqueue_side_A(ctx, s, a_from, first));
    HIPCHK(ctx, hipStreamWaitEvent(s.st, s.ev_R, 0));
    HIPCHK(ctx, hipGetLastError());
    s.have_pyr = !win && !direct0 && built == 0;
    return UGSM_OK;
}
int enqueue_pyramids(ugsm_ctx *ctx, Slot &s, int si, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int a_from, const FoveaWin *win, bool full)
{
    return enqueue_pyramids(ctx, s, si, &d_rgbL, &d_rgbR, 1, W, H, stride, a_from, win, full);
}

// Level `lev` + 1's fields (Ws x Hs, in `cur`) handed to level `lev` (W x H): subsampleDisp, MatchGPULib.cpp:1526-1590, and
// foveatedsubsampleDisp, :1595-1655.  Fills the entries' seed maps; where level `lev`'s first K-cost launch reads `cur` through them (fuse_seed)
// that is all: true.  Otherwise launch_seed writes the seeded fields into `other` and the two swap: false.
// g: the entries' fovea geometries, whose seed-crop origins of level `lev` apply; null (the full-frame levels): origin 0.
bool hand_seed(ugsm_ctx *ctx, Slot &s, int si, const Shape &sh, int Ws, int Hs, int W, int H, const FoveaGeom *g, int lev, SeedMap *sm, float *&cur,
               float *&other)
{
    for (int b = 0; b < sh.nb; b++) sm[b] = SeedMap{Ws, Hs, g ? g[b].cx[lev] : 0, g ? g[b].cy[lev] : 0};
    const int np = launch_pairs(ctx, sh, W, H);
    if (fuse_seed(ctx, W, H, s.alone, np)) return true;
    for_groups(sh.nb, np > 1, [&](Grp gr) {
        Timer t(ctx, &s, si, KC_SEED, (double)W * H * gr.n);
        const Batch bt = make_batch(sh, gr, nullptr, sm);
        launch_seed(s.st, cur + gr.b0 * sh.stride, Ws, Hs, other + gr.b0 * sh.stride, W, H, sm[gr.b0].cx, sm[gr.b0].cy, gr.n > 1 ? &bt : nullptr);
    });
    std::swap(cur, other);
    return false;
}

}  // namespace ugsm
