// ugsm_fovea_seeded.cpp -- the entry points of the seeded (warm) foveated call (include/ugsm.h: ugsm_submit_foveated_warm,
// ugsm_submit_foveated_warm_field, ugsm_match_foveated_warm, ugsm_fovea_warm_pixel_iterations): what the call refuses, all of it before
// anything is enqueued, and the call's size.  Written against the public entry points and ugsm_internal.hpp only (no HIP call here, as
// ugsm_seeded.cpp): the runtime does the enqueueing (ugsm::fovea_warm_submit: ugsm_fovea.cpp; ugsm::fovea_warm_match: ugsm_host.cpp), and the refusals
// can be driven on a machine without a GPU (tests/fake_fovea_seeded.cpp).
#include "ugsm_internal.hpp"

#include <stdint.h>

using namespace ugsm;

// What every form refuses beyond its null pointers: the shared refusals (refuse_common) around the call's own two, the context's fovea and the
// start level; the fovea's size comes back for the overlap test.
static int warm_check(ugsm_ctx *ctx, int n, int W, int H, int stride, int start_level, int *fw, int *fh)
{
    const ugsm_config &cfg = ctx_config(ctx);
    const int F = cfg.fovea_levels;
    const char *own = (F < 2 || F > cfg.levels)          ? "the warm foveated call needs a context with fovea_levels >= 2"
                      : (start_level < 0 || start_level >= F) ? "the warm foveated call: start_level outside 0 .. fovea_levels - 1"
                                                              : nullptr;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    const int st = refuse_common(ctx, "the warm foveated call", UGSM_LR_FOVEATED, n, own, W, H, stride, w, h);
    if (st != UGSM_OK) return st;
    *fw = w[F - 1];  // (ugsm_fovea_dims)
    *fh = h[F - 1];
    return UGSM_OK;
}

// field: the priors are full-resolution fields; else stacks, with their windows' offsets (null arrays: centred)
static int warm_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                       const int *off_x, const int *off_y, const float *const *d_prior, const int *prior_off_x, const int *prior_off_y, bool field,
                       int start_level, float *const *d_stack)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!d_rgbL || !d_rgbR || !d_prior || !d_stack) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the warm foveated call: a null array");
    int fw = 0, fh = 0;
    const int st = warm_check(ctx, n, W, H, stride, start_level, &fw, &fh);
    if (st != UGSM_OK) return st;
    for (int b = 0; b < n; b++)
        if (!d_rgbL[b] || !d_rgbR[b] || !d_prior[b] || !d_stack[b]) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the warm foveated call: a null entry");
    // not in place: the launch that reads the priors writes the stacks' upper row blocks
    const size_t stack_bytes = sizeof(float) * 3 * (size_t)ctx_config(ctx).fovea_levels * fw * fh;
    const size_t prior_bytes = field ? sizeof(float) * 3 * (size_t)W * H : stack_bytes;
    for (int a = 0; a < n; a++)
        for (int b = 0; b < n; b++)
            if (overlap(d_prior[a], prior_bytes, d_stack[b], stack_bytes))
                return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the warm foveated call is not in place: a prior is one of the call's d_stack buffers (alternate two stacks)");
    return fovea_warm_submit(ctx, slot, n, d_rgbL, d_rgbR, W, H, stride, off_x, off_y, d_prior, prior_off_x, prior_off_y, field ? 1 : 0, start_level, d_stack);
}

extern "C" {

int ugsm_submit_foveated_warm(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                              const int *off_x, const int *off_y, const float *const *d_prior_stack, const int *prior_off_x, const int *prior_off_y,
                              int start_level, float *const *d_stack)
{
    return warm_submit(ctx, slot, n, d_rgbL, d_rgbR, W, H, stride, off_x, off_y, d_prior_stack, prior_off_x, prior_off_y, false, start_level, d_stack);
}

int ugsm_submit_foveated_warm_field(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                                    const int *off_x, const int *off_y, const float *const *d_prior_field, int start_level, float *const *d_stack)
{
    return warm_submit(ctx, slot, n, d_rgbL, d_rgbR, W, H, stride, off_x, off_y, d_prior_field, nullptr, nullptr, true, start_level, d_stack);
}

int ugsm_match_foveated_warm(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y, const float *priorH,
                             const float *priorV, const float *priorC, int prior_off_x, int prior_off_y, int start_level, float *stackH, float *stackV,
                             float *stackC)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!rgbL || !rgbR || !priorH || !priorV || !priorC || !stackH || !stackV || !stackC)
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "the warm foveated call: a null pointer");
    int fw = 0, fh = 0;
    const int st = warm_check(ctx, 1, W, H, stride, start_level, &fw, &fh);
    if (st != UGSM_OK) return st;
    const float *const prior[3] = {priorH, priorV, priorC};
    float *const stack[3] = {stackH, stackV, stackC};
    return fovea_warm_match(ctx, rgbL, rgbR, W, H, stride, off_x, off_y, prior, prior_off_x, prior_off_y, start_level, stack);
}

long long ugsm_fovea_warm_pixel_iterations(int W, int H, int levels, int fovea_levels, int start_level)
{
    int fw = 0, fh = 0, w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    if (levels < 1 || levels > UGSM_MAX_LEVELS || fovea_levels < 2 || fovea_levels > levels || start_level < 0 || start_level >= fovea_levels) return -1;
    if (ugsm_level_dims(W, H, levels, w, h) != UGSM_OK || ugsm_fovea_dims(W, H, levels, fovea_levels, &fw, &fh) != UGSM_OK) return -1;
    long long tot = 0;
    for (int i = 0; i <= start_level; i++) tot += (long long)fw * fh * ugsm_level_iterations(i);
    return tot;
}

}  // extern "C"
