// ugsm_internal.hpp -- what the layers above the slot API (ugsm_queue.cpp: the queue; ugsm_shard.cpp: RCCL) need from the runtime
// besides include/ugsm.h itself.  Both are written against the public slot-level entry points (ugsm_submit_*, ugsm_wait, ugsm_poll,
// ugsm_slot_stream): they are what a host would otherwise have to write, moved behind the C-ABI.
#pragma once

#include "../../include/ugsm.h"

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <new>

namespace ugsm {

constexpr long long kMaxPixels = 1LL << 28;  // 268 Mpx: 4 B x pixels of one plane stays below 2^31

// Row f-1's rules, stated once for the slot-level calls (ugsm_cloud.cpp) and for the queue, which makes them when a pair is enqueued.
// The keep window of ugsm_cloud_params / ugsm_depth_params: no NaN among min_conf, z_min and z_max, z_min <= z_max, and no confidence
// test without a confidence plane (have_conf; the queue's pairs always have one).
inline bool keep_window_ok(float min_conf, float z_min, float z_max, bool have_conf)
{
    if (std::isnan(min_conf) || std::isnan(z_min) || std::isnan(z_max) || z_min > z_max) return false;
    return have_conf || !(min_conf > -INFINITY);
}
// ... and the records of ugsm_cloud_params: the sampling and the format
inline bool cloud_records_ok(const ugsm_cloud_params &p)
{
    return p.sampling >= 1 && (p.format == UGSM_CLOUD_PCL32 || p.format == UGSM_CLOUD_XYZRGB16);
}

// A call of n pairs with a cloud each (ugsm_enqueue_*_cloud*), as the queue hands it to the runtime through CtxHooks::cloud_submit.
struct CloudJob {
    const uint8_t *L, *R;  // device kind: the device images; managed: the page-locked staging
    int off_x, off_y;
    float *out;            // device kind: d_out / d_stack
    float *planes[3];      // managed with want_planes: the page-locked planes the pair's result goes to
    void *points;          // device kind: d_points, cap_points, d_count, d_level_counts
    long long cap;
    long long *count, *level_counts;
};
struct CloudCall {
    int fovea, managed, n, W, H, stride;
    const ugsm_queue_cloud *spec;  // the call's (every pair's) spec
    CloudJob job[UGSM_MAX_BATCH];
};

// A call of n checked full-mode pairs (ugsm_enqueue_full_checked*), as the queue hands it to the runtime through CtxHooks::checked_submit.
struct CheckedJob {
    const uint8_t *L, *R;   // device kind: the device images; managed: the page-locked staging
    float *out, *back;      // device kind: d_out, and d_back or null (the pair does not take the right camera's field)
    float *planes[3];       // managed: the page-locked planes of the checked forward field (null: a cloud pair without want_planes)
    float *back_planes[3];  // managed with want_back: those of the right camera's checked field
    void *points;           // device kind with a cloud: d_points, cap_points, d_count
    long long cap;
    long long *count;
};
struct CheckedCall {
    int managed, n, W, H, stride;
    float tau;                     // the call's (every pair's) threshold
    const ugsm_queue_cloud *spec;  // the call's (every pair's) cloud spec; null: pairs without a cloud
    CheckedJob job[UGSM_MAX_BATCH];
};

// State the layers hang on a context; the runtime owns the storage and calls the `free` hooks from ugsm_destroy (before the slots go).
struct CtxHooks {
    // The queue's way to the cloud work (set by ugsm_create; nullptr in a runtime that has none: tests/fake_runtime.cpp).  cloud_submit:
    // the match of the call's pairs as ugsm_submit_*_batch[_host] enqueues it, then their clouds, on the slot's stream; a managed call's counts
    // come down to page-locked words behind them.  cloud_finish (managed calls, once the slot has been seen idle after cloud_submit): reads
    // the counts into res[0 .. n), asks `staging(user, pair, bytes)` for page-locked memory of stored x point_step bytes per pair (nullptr: out
    // of memory) and enqueues the device-to-host copies on the slot's stream: the slot is busy again until they have drained.
    int (*cloud_submit)(ugsm_ctx *, int slot, const CloudCall *call) = nullptr;
    int (*cloud_finish)(ugsm_ctx *, int slot, int n, ugsm_cloud_result *res, void *(*staging)(void *user, int pair, long long bytes), void *user) = nullptr;
    // The queue's way to the checked full-mode call (set by ugsm_create; nullptr in a runtime that has none).  checked_submit: both directions
    // of the call's pairs in lockstep with the call's tau, as ugsm_submit_full_checked[_host] enqueues them -- a managed call's images up and
    // its planes down around the match -- and, with a spec, the clouds of the checked forward fields behind it on the slot's stream, as
    // cloud_submit puts them there (a managed call then finishes through cloud_finish).  checked_marked (once the slot has drained): the
    // pixels the check marked in each direction of the call's n pairs.
    int (*checked_submit)(ugsm_ctx *, int slot, const CheckedCall *call) = nullptr;
    int (*checked_marked)(ugsm_ctx *, int slot, int n, long long *fwd, long long *back) = nullptr;
    void *queue = nullptr;
    void (*queue_free)(ugsm_ctx *, void *) = nullptr;
    void *shard = nullptr;
    void (*shard_free)(ugsm_ctx *, void *) = nullptr;
    bool queue_busy = false;   // pairs are outstanding in the queue: the slots belong to it (slot-level entry points answer UGSM_ERR_STATE)
    bool queue_calling = false;  // ... except while the queue itself is calling them
    bool queue_more = false;     // (while queue_calling) other calls follow the one being sent: it shares the chip (call_alone)
    // The shard's part in ugsm_wait / ugsm_poll (block = 0) on a slot that holds a shard step: called BEFORE the runtime waits for the slot.
    // UGSM_OK: go on (wait / query the slot as usual); UGSM_PENDING: (poll) not finished; anything else is returned to the caller once the
    // slot has drained -- a peer rank failed its part of the step, or the step's deadline passed and the communicator was aborted.
    int (*shard_wait)(ugsm_ctx *, int slot, int block) = nullptr;
    // ugsm_set_input_format: the format of the images the next calls hand over (the queue stores it with each pair and sets it back while
    // it sends the pair's call)
    int input_format = UGSM_INPUT_RGB8;
    // ugsm_set_lens: a lens is set.  The queue's cloud pairs and the merged cloud of several windows refuse then (include/ugsm.h, "lens
    // distortion"); the values themselves are the runtime's.
    bool lens_set = false;
};
// ugsm_input_bytes_per_pixel: 3, 3, 4, 4, 1 for UGSM_INPUT_RGB8 .. UGSM_INPUT_MONO8, -1 otherwise
inline int input_bpp(int format)
{
    switch (format) {
    case UGSM_INPUT_RGB8:
    case UGSM_INPUT_BGR8: return 3;
    case UGSM_INPUT_RGBA8:
    case UGSM_INPUT_BGRA8: return 4;
    case UGSM_INPUT_MONO8: return 1;
    case UGSM_INPUT_RGB32F: return 12;
    case UGSM_INPUT_MONO32F: return 4;
    default: return -1;
    }
}
inline bool input_float(int format) { return format == UGSM_INPUT_RGB32F || format == UGSM_INPUT_MONO32F; }
// The one check of an image's rows and base pointers against the input format, which every entry point that takes an image passes
// through before it enqueues anything: UGSM_ERR_SIZE_MISMATCH for stride < bytes per pixel * W; for a float format UGSM_ERR_BAD_ARG for a
// stride that is no multiple of 4 or an image pointer (a or b; null: not looked at) that is not 4-byte aligned -- the kernels read a
// float pixel with dword loads.
inline int input_image_status(int format, int W, int stride, const void *a = nullptr, const void *b = nullptr)
{
    if ((long long)stride < (long long)input_bpp(format) * W) return UGSM_ERR_SIZE_MISMATCH;
    if (!input_float(format)) return UGSM_OK;
    return ((stride & 3) || (reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(b) & 3)) ? UGSM_ERR_BAD_ARG : UGSM_OK;
}
CtxHooks &ctx_hooks(ugsm_ctx *ctx);
const ugsm_config &ctx_config(const ugsm_ctx *ctx);
// the HIP stream of a slot (a hipStream_t), nullptr for a slot the context does not have; unlike ugsm_slot_stream it leaves the slot's
// bookkeeping alone (the public call takes it that the host is about to enqueue work of its own there: the slot becomes busy)
void *ctx_slot_stream(ugsm_ctx *ctx, int slot);
// sets ugsm_last_error and returns `status`
int ctx_fail(ugsm_ctx *ctx, int status, const char *what);
// memcpy by the context's host team (large copies; falls back to the calling thread)
void ctx_host_copy(ugsm_ctx *ctx, void *dst, const void *src, size_t bytes);
// hipPointerGetAttributes says page-locked host memory
bool host_pinned(const void *p);
// UGSM_DEV=1 is set: the process asked for the development switches (UGSM_* environment variables); nothing reads one without it
bool dev_env();
// The seeded full-mode call behind its entry points (ugsm_seeded.cpp, which has refused what the call refuses): n pairs enqueued on `slot`
// from level start_level of their priors; and the blocking call on slot 0, its three prior and result planes in host memory of any kind.
int seeded_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                  const float *const *d_prior, int start_level, float *const *d_out);
int seeded_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const float *const prior[3], int start_level,
                 float *const disp[3]);
// The warm foveated call behind its entry points (ugsm_fovea_seeded.cpp, which has refused what the call refuses): n pairs enqueued on `slot`
// from fovea level start_level of their priors -- stacks with their windows' offsets (null arrays: centred), or, field != 0, full-resolution
// fields --; and the blocking call on slot 0, its three prior and result stack planes in host memory of any kind.
int fovea_warm_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride, const int *off_x,
                      const int *off_y, const float *const *d_prior, const int *prior_off_x, const int *prior_off_y, int field, int start_level,
                      float *const *d_stack);
int fovea_warm_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y, const float *const prior[3],
                     int prior_off_x, int prior_off_y, int start_level, float *const stack[3]);
// The full-mode call in two halves behind its entry points (ugsm_coarse.cpp, which has refused what the calls refuse): n pairs enqueued on
// `slot` -- the levels top .. stop_level into d_state, prolonged into the d_full entries that are set (d_full may be null); the levels
// state_level - 1 .. 0 from d_state into d_out --; and the blocking calls on slot 0, their planes in host memory of any kind (full: null for none).
int coarse_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride, int stop_level,
                  float *const *d_state, float *const *d_full);
int fine_submit(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *d_rgbL, const uint8_t *const *d_rgbR, int W, int H, int stride,
                const float *const *d_state, int state_level, float *const *d_out);
int coarse_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int stop_level, float *const state[3],
                 float *const full[3]);
int fine_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const float *const state[3], int state_level,
               float *const disp[3]);
// What the seeded call, the two halves and the warm foveated call all refuse beyond their null pointers (ugsm_seeded.cpp, ugsm_coarse.cpp,
// ugsm_fovea_seeded.cpp), in the one order they have always had: the pair count, the call's own refusal of its level arguments, the early
// exit, a busy queue, the LR check, a size with no pyramid, a stride too small.
// what: the call's name for the messages; lr_mode: the UGSM_LR_* bit under which the call has no checked form; own: the message of the call's own
// refusal (null: its level arguments are fine); the levels' sizes come back in w and h.
inline int refuse_common(ugsm_ctx *ctx, const char *what, int lr_mode, int n, const char *own, int W, int H, int stride, int *w, int *h)
{
    const ugsm_config &cfg = ctx_config(ctx);
    const CtxHooks &hooks = ctx_hooks(ctx);
    char msg[200];
    snprintf(msg, sizeof msg, "%s takes 1 .. UGSM_MAX_BATCH pairs", what);
    if (n < 1 || n > UGSM_MAX_BATCH) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, msg);
    if (own) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, own);
    // (the early exit compares a level's fields pair by pair through a third buffer and a host round trip per iteration: no lockstep, a level's
    // field then depends on the exit, and it is no use beside a prior)
    snprintf(msg, sizeof msg, "%s: not with early_exit_threshold > 0", what);
    if (cfg.early_exit_threshold > 0.0f) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, msg);
    if (hooks.queue_busy && !hooks.queue_calling)
        return ctx_fail(ctx, UGSM_ERR_STATE, "pairs enqueued with ugsm_enqueue_* are outstanding: the slots belong to the queue until ugsm_next_done has reported them all");
    float tau = 0.0f;
    int modes = 0;
    snprintf(msg, sizeof msg, "the %s LR check is on (ugsm_set_lr_check): %s has no checked form", lr_mode == UGSM_LR_FULL ? "full-mode" : "foveated", what);
    if (ugsm_get_lr_check(ctx, &tau, &modes) == UGSM_OK && tau > 0.0f && (modes & lr_mode)) return ctx_fail(ctx, UGSM_ERR_STATE, msg);
    const int st = ugsm_level_dims(W, H, cfg.levels, w, h);
    if (st != UGSM_OK) return st;
    return input_image_status(hooks.input_format, W, stride);
}
// two buffers of abytes and bbytes share a byte
inline bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}
// the stagger of the queue's first round after idle and the size of every later call (ugsm.h, "the queue")
int queue_target(int batch, int slots, long long calls_since_idle);

// The body of a C entry point that uses growing containers: nothing is thrown across the C-ABI.
template <class F>
int no_throw(ugsm_ctx *ctx, const char *entry, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return ctx ? ctx_fail(ctx, UGSM_ERR_NOMEM, entry) : UGSM_ERR_NOMEM;
    } catch (...) {
        return ctx ? ctx_fail(ctx, UGSM_ERR_STATE, entry) : UGSM_ERR_STATE;
    }
}

}  // namespace ugsm
