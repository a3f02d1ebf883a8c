// ugsm_stages.cpp -- the stage-level entry points, ugsm_stage_* (tests only): one stage of the matcher at a time, on slot 0, blocking.
#include "../../include/ugsm.h"
#include "ugsm_device.hpp"
#include "ugsm_slot.hpp"

#include <algorithm>

using namespace ugsm;

extern "C" {

int ugsm_stage_pyramid(ugsm_ctx *ctx, const uint8_t *d_rgb, int W, int H, int stride, int level, float *d_out3)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_rgb || !d_out3 || level < 0 || level >= ctx->cfg.levels) return UGSM_ERR_BAD_ARG;
    UCHK(input_status(ctx, W, stride, d_rgb));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(prepare_slot(ctx, *s, W, H));
    UCHK(build_pyramids(ctx, *s, 0, &d_rgb, stride, s->pyrL));
    HIPCHK(ctx, hipMemcpyAsync(d_out3, s->pyrL + s->off[level], sizeof(float) * 3 * (size_t)s->w[level] * s->h[level],
                               hipMemcpyDeviceToDevice, s->st));
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_iterate(ugsm_ctx *ctx, const float *d_L3, const float *d_R3, float *d_d3, int W, int H, int mi, int S,
                       int is_top, int m_from, int m_to, float *d_dbg8)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_L3 || !d_R3 || !d_d3 || W < 1 || H < 1 || mi < 1 || m_from < 1 || m_to > mi || S < 0) return UGSM_ERR_BAD_ARG;
    if ((long long)W * H > kMaxPixels) return UGSM_ERR_BAD_ARG;
    if (d_dbg8 && ctx->cfg.kernel_path != 1) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    // level buffers sized for this image; the pyramid buffers are not needed here
    const size_t lvl = 3 * (size_t)W * H;
    UCHK(ensure_level_bufs(ctx, *s, lvl));
    float *cur = s->d0, *other = s->d1;
    HIPCHK(ctx, hipMemcpyAsync(cur, d_d3, lvl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    const size_t n = (size_t)W * H;
    // the planes arrive ready-made: check their range here (the pyramid kernels do it for the matcher proper).  The slot's range
    // word then describes THESE planes, no longer the slot's pyramids: a fovea phase submitted afterwards must rebuild them first
    s->have_pyr = false;
    s->range_known = ctx->cfg.kernel_path != 1;
    if (s->range_known) {
        HIPCHK(ctx, hipMemsetAsync(s->range_bad, 0, sizeof(unsigned), s->st));
        launch_range_scan(s->st, d_L3, 3 * n, s->range_bad);
        launch_range_scan(s->st, d_R3, 3 * n, s->range_bad);
    }
    s->nb = 1;
    const Img3 Lv{d_L3, W, n}, Rv{d_R3, W, n};
    UCHK(run_level(ctx, *s, 0, Shape::pairs(*s), &Lv, &Rv, W, H, mi, S, is_top != 0, m_from, m_to, cur, other, d_dbg8));
    HIPCHK(ctx, hipMemcpyAsync(d_d3, cur, lvl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_seed(ugsm_ctx *ctx, const float *d_src3, int W, int H, float *d_dst3, int W2, int H2, int Wup, int Hup,
                    int crop_x, int crop_y)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_src3 || !d_dst3 || W < 1 || H < 1 || W2 < 1 || H2 < 1) return UGSM_ERR_BAD_ARG;
    (void)Wup;
    (void)Hup;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    {
        Timer t(ctx, s, 0, KC_SEED, (double)W2 * H2);  // (profile_events = 2: the launch's own duration in the kernel statistics)
        launch_seed(s->st, d_src3, W, H, d_dst3, W2, H2, crop_x, crop_y);
    }
    HIPCHK(ctx, hipGetLastError());
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_restrict(ugsm_ctx *ctx, const float *d_src3, int W, int H, int level, float *d_dst3)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_src3 || !d_dst3 || level < 0 || level >= ctx->cfg.levels) return UGSM_ERR_BAD_ARG;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    launch_restrict(s->st, d_src3, W, H, level, d_dst3, w[level], h[level]);
    HIPCHK(ctx, hipGetLastError());
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_prolong(ugsm_ctx *ctx, const float *d_src3, int W, int H, int level, float *d_dst3)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_src3 || !d_dst3 || level < 0 || level >= ctx->cfg.levels) return UGSM_ERR_BAD_ARG;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    s->cur_level = level;
    bool launched;
    {
        Timer t(ctx, s, 0, KC_PROLONG, (double)W * H);
        launched = launch_prolong(s->st, d_src3, w, h, level, d_dst3);
    }
    if (!launched) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the prolongation: a size its kernel does not cover");
    HIPCHK(ctx, hipGetLastError());
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_warm_stack(ugsm_ctx *ctx, const float *d_prior_stack, int W, int H, int prior_off_x, int prior_off_y, int off_x, int off_y, int start_level,
                          float *d_dst_stack)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    const int F = ctx->cfg.fovea_levels;
    if (!d_prior_stack || !d_dst_stack || d_prior_stack == d_dst_stack || F < 2 || F > ctx->cfg.levels || start_level < 0 || start_level >= F) return UGSM_ERR_BAD_ARG;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(enqueue_restrict_stack(ctx, *s, 0, 1, w, h, F, &d_prior_stack, &prior_off_x, &prior_off_y, false, &off_x, &off_y, start_level, &d_dst_stack, nullptr, 0));
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_smooth(ugsm_ctx *ctx, float *d_d3, int W, int H, int passes, int do_box)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_d3 || W < 1 || H < 1 || passes < 0 || (long long)W * H > kMaxPixels) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const size_t lvl = 3 * (size_t)W * H;
    UCHK(ensure_level_bufs(ctx, *s, lvl));
    float *a = s->d0, *b = s->d1;
    HIPCHK(ctx, hipMemcpyAsync(a, d_d3, lvl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    s->nb = 1;
    UCHK(enqueue_smooth(ctx, *s, 0, Shape::pairs(*s), a, b, W, H, passes, do_box != 0));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(d_d3, a, lvl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_weighted_difference(ugsm_ctx *ctx, const float *d_new3, const float *d_old3, int W, int H, float *out2)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_new3 || !d_old3 || !out2 || W < 1 || H < 1 || H > 65535 || (long long)W * H > kMaxPixels) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    return weighted_difference(ctx, *s, d_new3, d_old3, W, H, out2);
}

int ugsm_stage_lr_check(ugsm_ctx *ctx, float *d_left3, const float *d_right3, int W, int H, float tau, long long *marked)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_left3 || !d_right3 || W < 1 || H < 1 || H > 65535 || (long long)W * H > kMaxPixels || !(tau >= 0.0f)) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(lr_ready(ctx, *s, std::max<size_t>(s->lr.cap, 8)));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(s->lr.p);
    HIPCHK(ctx, hipStreamSynchronize(s->st));  // (the counter shares the slot's LR buffer)
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof *cnt, s->st));
    launch_lr_check(s->st, d_left3, d_right3, W, H, tau, cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(s->lr_host, cnt, sizeof *cnt, hipMemcpyDeviceToHost, s->st));
    UCHK(ugsm_wait(ctx, 0));
    if (marked) *marked = (long long)*s->lr_host;
    return UGSM_OK;
}

}  // extern "C"
