// ugsm_seeded.cpp -- the entry points of the seeded full-mode call (include/ugsm.h: ugsm_submit_full_seeded, ugsm_match_full_seeded,
// ugsm_seeded_pixel_iterations): what the call refuses, all of it before anything is enqueued, and the call's size.  Written against the
// public entry points and ugsm_internal.hpp only (no HIP call here, as the queue): the runtime does the enqueueing (ugsm::seeded_submit:
// ugsm_full.cpp; ugsm::seeded_match: ugsm_host.cpp), and the refusals can be driven on a machine without a GPU (tests/fake_seeded.cpp).
#include "ugsm_internal.hpp"

using namespace ugsm;

// What both calls refuse beyond their null pointers: the shared refusals (refuse_common) around the call's own level.
static int seeded_check(ugsm_ctx *ctx, int n, int W, int H, int stride, int start_level)
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    const bool bad = start_level < 0 || start_level >= ctx_config(ctx).levels;
    return refuse_common(ctx, "the seeded full-mode call", UGSM_LR_FULL, n, bad ? "the seeded full-mode call: start_level outside 0 .. levels - 1" : nullptr, W, H,
                         stride, w, h);
}

extern "C" {

int ugsm_submit_full_seeded(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                            const float *const *d_prior, int start_level, float *const *d_out)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!d_rgbL || !d_rgbR || !d_prior || !d_out) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the seeded full-mode call: a null array");
    const int st = seeded_check(ctx, n, W, H, stride, start_level);
    if (st != UGSM_OK) return st;
    for (int b = 0; b < n; b++)
        if (!d_rgbL[b] || !d_rgbR[b] || !d_prior[b] || !d_out[b]) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the seeded full-mode call: a null entry");
    return seeded_submit(ctx, slot, n, d_rgbL, d_rgbR, W, H, stride, d_prior, start_level, d_out);
}

int ugsm_match_full_seeded(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const float *priorH, const float *priorV,
                           const float *priorC, int start_level, float *dispH, float *dispV, float *dispC)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!rgbL || !rgbR || !priorH || !priorV || !priorC || !dispH || !dispV || !dispC)
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the seeded full-mode call: a null pointer");
    const int st = seeded_check(ctx, 1, W, H, stride, start_level);
    if (st != UGSM_OK) return st;
    const float *const prior[3] = {priorH, priorV, priorC};
    float *const disp[3] = {dispH, dispV, dispC};
    return seeded_match(ctx, rgbL, rgbR, W, H, stride, prior, start_level, disp);
}

long long ugsm_seeded_pixel_iterations(int W, int H, int levels, int start_level)
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    if (levels < 1 || levels > UGSM_MAX_LEVELS || start_level < 0 || start_level >= levels) return -1;
    if (ugsm_level_dims(W, H, levels, w, h) != UGSM_OK) return -1;
    long long tot = 0;
    for (int i = 0; i <= start_level; i++) tot += (long long)w[i] * h[i] * ugsm_level_iterations(i);
    return tot;
}

}  // extern "C"
