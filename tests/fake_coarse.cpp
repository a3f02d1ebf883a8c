// Test infrastructure (tests/test_coarse_host.py): what csrc/ugsm_coarse.cpp -- the entry points of the full-mode call in two halves, which
// refuse what the calls refuse before the runtime enqueues anything -- needs underneath it beyond the recording stand-in runtime
// (tests/fake_runtime.cpp, unchanged): the LR setting of a context, the iteration counts, setters for the three things the refusals look at,
// and recorders in place of ugsm::coarse_submit / fine_submit / coarse_match / fine_match, which count how often the runtime would have been
// reached.
#include "../ug_stereomatcher_amd/csrc/ugsm_internal.hpp"

static float g_tau = 0.0f;
static int g_modes = 0, g_reached[4] = {0, 0, 0, 0}, g_last[5] = {0, 0, 0, 0, 0};

static int reached(int which, int slot, int n, int W, int level, int full)
{
    g_reached[which]++;
    g_last[0] = slot;
    g_last[1] = n;
    g_last[2] = W;
    g_last[3] = level;
    g_last[4] = full;
    return UGSM_OK;
}

namespace ugsm {
int coarse_submit(ugsm_ctx *, int slot, int n, const uint8_t *const *, const uint8_t *const *, int W, int, int, int stop_level, float *const *, float *const *d_full)
{
    int full = 0;
    for (int b = 0; d_full && b < n; b++) full += d_full[b] != nullptr;
    return reached(0, slot, n, W, stop_level, full);
}
int fine_submit(ugsm_ctx *, int slot, int n, const uint8_t *const *, const uint8_t *const *, int W, int, int, const float *const *, int state_level, float *const *)
{
    return reached(1, slot, n, W, state_level, 0);
}
int coarse_match(ugsm_ctx *, const uint8_t *, const uint8_t *, int W, int, int, int stop_level, float *const[3], float *const full[3])
{
    return reached(2, 0, 1, W, stop_level, full ? 1 : 0);
}
int fine_match(ugsm_ctx *, const uint8_t *, const uint8_t *, int W, int, int, const float *const[3], int state_level, float *const[3])
{
    return reached(3, 0, 1, W, state_level, 0);
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
void ugsm_fake_coarse_lr(float tau, int modes)
{
    g_tau = tau;
    g_modes = modes;
}
void ugsm_fake_coarse_early_exit(ugsm_ctx *ctx, float eps) { const_cast<ugsm_config &>(ugsm::ctx_config(ctx)).early_exit_threshold = eps; }
void ugsm_fake_coarse_queue_busy(ugsm_ctx *ctx, int busy) { ugsm::ctx_hooks(ctx).queue_busy = busy != 0; }
void ugsm_fake_coarse_input_format(ugsm_ctx *ctx, int format) { ugsm::ctx_hooks(ctx).input_format = format; }
// calls that reached the runtime: coarse submits, fine submits, blocking coarse, blocking fine; and of the last one: slot, pairs, W, level,
// d_full entries set
void ugsm_fake_coarse_reached(int *out9)
{
    for (int k = 0; k < 4; k++) out9[k] = g_reached[k];
    for (int k = 0; k < 5; k++) out9[4 + k] = g_last[k];
}
#pragma GCC visibility pop
}
