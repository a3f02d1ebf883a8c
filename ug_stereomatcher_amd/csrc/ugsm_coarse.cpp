// ugsm_coarse.cpp -- the entry points of the full-mode call in two halves (include/ugsm.h: ugsm_submit_full_coarse, ugsm_submit_full_fine,
// ugsm_match_full_coarse, ugsm_match_full_fine, ugsm_coarse_pixel_iterations): what the calls refuse, all of it before anything is enqueued,
// and the coarse half's size.  Written against the public entry points and ugsm_internal.hpp only (no HIP call here, as ugsm_seeded.cpp): the
// runtime does the enqueueing (ugsm::coarse_submit, fine_submit: ugsm_full.cpp; coarse_match, fine_match: ugsm_host.cpp), and the refusals can be driven
// on a machine without a GPU (tests/fake_coarse.cpp).
#include "ugsm_internal.hpp"

#include <stdint.h>

using namespace ugsm;

// What the four calls refuse beyond their null pointers.  level: stop_level (lowest = 0) or state_level (lowest = 1); the level's size comes
// back in *we x *he.
static int halves_check(ugsm_ctx *ctx, int n, int W, int H, int stride, int level, int lowest, const char *bad_level, int *we, int *he)
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    const bool bad = level < lowest || level >= ctx_config(ctx).levels;
    const int st = refuse_common(ctx, "a full-mode call in two halves", UGSM_LR_FULL, n, bad ? bad_level : nullptr, W, H, stride, w, h);
    if (st != UGSM_OK) return st;
    *we = w[level];
    *he = h[level];
    return UGSM_OK;
}
static const char kBadStop[] = "ugsm_submit_full_coarse: stop_level outside 0 .. levels - 1";
static const char kBadState[] = "ugsm_submit_full_fine: state_level outside 1 .. levels - 1";

extern "C" {

int ugsm_submit_full_coarse(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                            int stop_level, float *const *d_state, float *const *d_full)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!d_rgbL || !d_rgbR || !d_state) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_submit_full_coarse: a null array");
    int we, he;
    const int st = halves_check(ctx, n, W, H, stride, stop_level, 0, kBadStop, &we, &he);
    if (st != UGSM_OK) return st;
    for (int b = 0; b < n; b++)
        if (!d_rgbL[b] || !d_rgbR[b] || !d_state[b]) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_submit_full_coarse: a null entry");
    // (the prolongation reads the states while it writes: an output that lies over any pair's state would be read half written)
    for (int b = 0; d_full && b < n; b++)
        for (int k = 0; d_full[b] && k < n; k++)
            if (overlap(d_full[b], sizeof(float) * 3 * (size_t)W * H, d_state[k], sizeof(float) * 3 * (size_t)we * he))
                return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_submit_full_coarse: a d_full entry overlaps a state of the call");
    return coarse_submit(ctx, slot, n, d_rgbL, d_rgbR, W, H, stride, stop_level, d_state, d_full);
}

int ugsm_submit_full_fine(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                          const float *const *d_state, int state_level, float *const *d_out)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!d_rgbL || !d_rgbR || !d_state || !d_out) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_submit_full_fine: a null array");
    int we, he;
    const int st = halves_check(ctx, n, W, H, stride, state_level, 1, kBadState, &we, &he);
    if (st != UGSM_OK) return st;
    for (int b = 0; b < n; b++)
        if (!d_rgbL[b] || !d_rgbR[b] || !d_state[b] || !d_out[b]) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_submit_full_fine: a null entry");
    return fine_submit(ctx, slot, n, d_rgbL, d_rgbR, W, H, stride, d_state, state_level, d_out);
}

int ugsm_match_full_coarse(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int stop_level, float *stateH, float *stateV,
                           float *stateC, float *fullH, float *fullV, float *fullC)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!rgbL || !rgbR || !stateH || !stateV || !stateC) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_match_full_coarse: a null pointer");
    const int given = (fullH != nullptr) + (fullV != nullptr) + (fullC != nullptr);
    if (given != 0 && given != 3) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_match_full_coarse: the three full-resolution planes, or none");
    int we, he;
    const int st = halves_check(ctx, 1, W, H, stride, stop_level, 0, kBadStop, &we, &he);
    if (st != UGSM_OK) return st;
    float *const state[3] = {stateH, stateV, stateC};
    float *const full[3] = {fullH, fullV, fullC};
    return coarse_match(ctx, rgbL, rgbR, W, H, stride, stop_level, state, given ? full : nullptr);
}

int ugsm_match_full_fine(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const float *stateH, const float *stateV,
                         const float *stateC, int state_level, float *dispH, float *dispV, float *dispC)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (!rgbL || !rgbR || !stateH || !stateV || !stateC || !dispH || !dispV || !dispC)
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_match_full_fine: a null pointer");
    int we, he;
    const int st = halves_check(ctx, 1, W, H, stride, state_level, 1, kBadState, &we, &he);
    if (st != UGSM_OK) return st;
    const float *const state[3] = {stateH, stateV, stateC};
    float *const disp[3] = {dispH, dispV, dispC};
    return fine_match(ctx, rgbL, rgbR, W, H, stride, state, state_level, disp);
}

long long ugsm_coarse_pixel_iterations(int W, int H, int levels, int stop_level)
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    if (levels < 1 || levels > UGSM_MAX_LEVELS || stop_level < 0 || stop_level >= levels) return -1;
    if (ugsm_level_dims(W, H, levels, w, h) != UGSM_OK) return -1;
    long long tot = 0;
    for (int i = stop_level; i < levels; i++) tot += (long long)w[i] * h[i] * ugsm_level_iterations(i);
    return tot;
}

}  // extern "C"
