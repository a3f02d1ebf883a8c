// ugsm_dev_entries.cpp -- linked into libugsm_dev.so only: its answer to "which library is this", and the entry points of include/ugsm_dev.h
// (tests only): the probe kernels, the slot's range words and level-0 form, one level from rgb8 images.  On slot 0, blocking, as ugsm_stage_*.
#include "../../../include/ugsm.h"
#include "../../../include/ugsm_dev.h"
#include "../ugsm_device.hpp"
#include "../ugsm_slot.hpp"

using namespace ugsm;

namespace ugsm {
const bool kDevLib = true;
}

extern "C" {

int ugsm_stage_poly_probe(ugsm_ctx *ctx, const float *d_c, const float *d_l, const float *d_r, const float *d_thr, float *d_delta,
                          float *d_corr, float *d_third, int n)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_c || !d_l || !d_r || !d_thr || !d_delta || !d_corr || !d_third || n < 1) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    launch_poly_probe(s->st, d_c, d_l, d_r, d_thr, d_delta, d_corr, d_third, n);
    HIPCHK(ctx, hipGetLastError());
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_div_probe(ugsm_ctx *ctx, const float *d_n, const float *d_d, float *d_q, int n)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_n || !d_d || !d_q || n < 1) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    launch_div_probe(s->st, d_n, d_d, d_q, n);
    HIPCHK(ctx, hipGetLastError());
    return ugsm_wait(ctx, 0);
}

// The range words of the slot's last call (Slot::range_bad: zeroed by enqueue_pyramids, set by the pyramid kernels, read by the
// marching K-cost kernels), for the tests that drive that mechanism through whole calls.  Reads host state and device memory only:
// the slot does not become busy, nothing is launched.
int ugsm_stage_range_words(ugsm_ctx *ctx, int slot, unsigned *host_out, int n)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s, false));
    if (!host_out || n < 1 || n > kMaxBatch) return UGSM_ERR_BAD_ARG;
    if (!s->range_known || !s->range_bad) {
        ctx->err = "the slot holds no range words (kernel_path 1, or no call has built pyramids on it)";
        return UGSM_ERR_STATE;
    }
    if (n > s->nb) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    HIPCHK(ctx, hipStreamSynchronize(s->st));  // (the main stream has joined whatever the call put on the side stream)
    HIPCHK(ctx, hipMemcpy(host_out, s->range_bad, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    return UGSM_OK;
}

// Whether the last call on the slot read level 0 from the images (Slot::direct0) -- batched and queue-formed calls included, which leave no other
// trace of it: the results are the same bits either way.  Host state only.
int ugsm_stage_level0_direct(ugsm_ctx *ctx, int slot)
{
    Slot *s;
    const int st = get_slot(ctx, slot, &s, false);
    if (st != UGSM_OK) return -st;
    return s->direct0 ? 1 : 0;
}

// ugsm_stage_iterate with the two images given as rgb8 instead of float planes: the level runs the way level 0 of a full-mode call runs
// (Slot::direct0) -- A and K-cost through their 8-bit instances, on byte views of the images -- but from the caller's field, so that a test
// can send disparities of its own choosing through the clamped byte gather.
int ugsm_stage_iterate_rgb8(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int stride, float *d_d3, int W, int H, int mi, int S, int is_top,
                            int m_from, int m_to)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_rgbL || !d_rgbR || !d_d3 || W < 1 || H < 1 || mi < 1 || m_from < 1 || m_to > mi || S < 0) return UGSM_ERR_BAD_ARG;
    if ((long long)W * H > kMaxPixels || ctx->cfg.kernel_path == 1 || ctx->hooks.input_format != kInRGB8) return UGSM_ERR_BAD_ARG;
    if (stride < 3 * W) return UGSM_ERR_SIZE_MISMATCH;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const size_t lvl = 3 * (size_t)W * H;
    UCHK(ensure_level_bufs(ctx, *s, lvl));
    float *cur = s->d0, *other = s->d1;
    HIPCHK(ctx, hipMemcpyAsync(cur, d_d3, lvl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    s->have_pyr = false;
    s->range_known = true;  // (the integers 0 .. 255: always inside range_ok)
    HIPCHK(ctx, hipMemsetAsync(s->range_bad, 0, sizeof(unsigned), s->st));
    s->nb = 1;
    s->direct0 = false;  // (no call of the slot's: ugsm_stage_level0_direct)
    const Img3 Lv = byte_view(d_rgbL, stride), Rv = byte_view(d_rgbR, stride);
    UCHK(run_level(ctx, *s, 0, Shape::pairs(*s), &Lv, &Rv, W, H, mi, S, is_top != 0, m_from, m_to, cur, other, nullptr, nullptr, nullptr, nullptr, kInRGB8));
    HIPCHK(ctx, hipMemcpyAsync(d_d3, cur, lvl * sizeof(float), hipMemcpyDeviceToDevice, s->st));
    return ugsm_wait(ctx, 0);
}

int ugsm_stage_div3_probe(ugsm_ctx *ctx, const float *d_a0, const float *d_a1, const float *d_a2, const float *d_s, float *d_q0, float *d_q1,
                          float *d_q2, int n)
{
    Slot *s;
    UCHK(get_slot(ctx, 0, &s));
    if (!d_a0 || !d_a1 || !d_a2 || !d_s || !d_q0 || !d_q1 || !d_q2 || n < 1) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    launch_div3_probe(s->st, d_a0, d_a1, d_a2, d_s, d_q0, d_q1, d_q2, n);
    HIPCHK(ctx, hipGetLastError());
    return ugsm_wait(ctx, 0);
}

}  // extern "C"
