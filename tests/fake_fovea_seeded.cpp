// Test infrastructure (tests/test_fovea_seeded_host.py): what csrc/ugsm_fovea_seeded.cpp -- the entry points of the seeded (warm) foveated
// call, which refuse what the call refuses before the runtime enqueues anything -- needs underneath it beyond the recording stand-in runtime
// (tests/fake_runtime.cpp, unchanged): the LR setting of a context, the iteration counts, setters for the things the refusals look at, and
// recorders in place of ugsm::fovea_warm_submit / ugsm::fovea_warm_match, which count how often the runtime would have been reached.
#include "../ug_stereomatcher_amd/csrc/ugsm_internal.hpp"

static float g_tau = 0.0f;
static int g_modes = 0, g_submits = 0, g_matches = 0, g_last[5] = {0, 0, 0, 0, 0};

namespace ugsm {
int fovea_warm_submit(ugsm_ctx *, int slot, int n, const uint8_t *const *, const uint8_t *const *, int W, int, int, const int *, const int *, const float *const *,
                      const int *, const int *, int field, int start_level, float *const *)
{
    g_submits++;
    g_last[0] = slot;
    g_last[1] = n;
    g_last[2] = W;
    g_last[3] = start_level;
    g_last[4] = field;
    return UGSM_OK;
}
int fovea_warm_match(ugsm_ctx *, const uint8_t *, const uint8_t *, int W, int, int, int, int, const float *const[3], int, int, int start_level, float *const[3])
{
    g_matches++;
    g_last[0] = 0;
    g_last[1] = 1;
    g_last[2] = W;
    g_last[3] = start_level;
    g_last[4] = 0;
    return UGSM_OK;
}
}  // namespace ugsm

extern "C" {
int ugsm_get_lr_check(const ugsm_ctx *ctx, float *tau, int *modes)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    if (tau) *tau = g_tau;
    if (modes) *modes = g_modes;
    return UGSM_OK;
}
int ugsm_level_iterations(int level) { return level < 0 ? 0 : 2 + level; }  // (any rule: the test sums the same one)

#pragma GCC visibility push(default)
void ugsm_fake_warm_lr(float tau, int modes)
{
    g_tau = tau;
    g_modes = modes;
}
void ugsm_fake_warm_early_exit(ugsm_ctx *ctx, float eps) { const_cast<ugsm_config &>(ugsm::ctx_config(ctx)).early_exit_threshold = eps; }
void ugsm_fake_warm_fovea_levels(ugsm_ctx *ctx, int F) { const_cast<ugsm_config &>(ugsm::ctx_config(ctx)).fovea_levels = F; }
void ugsm_fake_warm_queue_busy(ugsm_ctx *ctx, int busy) { ugsm::ctx_hooks(ctx).queue_busy = busy != 0; }
void ugsm_fake_warm_input_format(ugsm_ctx *ctx, int format) { ugsm::ctx_hooks(ctx).input_format = format; }
// calls that reached the runtime: submits, blocking matches; and of the last one: slot, pairs, W, start_level, field
void ugsm_fake_warm_reached(int *out7)
{
    out7[0] = g_submits;
    out7[1] = g_matches;
    for (int k = 0; k < 5; k++) out7[2 + k] = g_last[k];
}
#pragma GCC visibility pop
}
