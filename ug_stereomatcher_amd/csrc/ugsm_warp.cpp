// ugsm_warp.cpp -- the warped right image (MatchGPULib::warpRightImage, MatchGPULib.cpp:1445-1518) and the photometric residual of a match
// (row f-4's rule, weightedDifference :1336-1437, on a left plane and the warped right plane), on the slots of ugsm_runtime.cpp.  Five
// slot-level entry points behind one preamble (warp_begin); the kernels are k_warp_right and k_residual_rows /
// k_residual_total (ugsm_kernels_warp.hip).  Definitions: include/ugsm.h.
#include "ugsm_slot.hpp"

using namespace ugsm;

namespace {

constexpr int kMaxWarpPlanes = 96;  // = 3 x UGSM_MAX_LEVELS: the grid's z of the stack form
constexpr int kMaxGridRows = 65535; // the grid's y is the image row

// the checks every entry point shares (no device needed)
bool shape_ok(int W, int H) { return W >= 1 && H >= 1 && H <= kMaxGridRows && (long long)W * H <= kMaxPixels; }

// What every entry point does before its launch: it takes the slot (UGSM_ERR_STATE while the queue holds it) and sets the device; a
// residual also makes the slot's row-sum scratch hold `rows` x 4 doubles, waiting for the stream only where the buffer is replaced.
int warp_begin(ugsm_ctx *ctx, int slot, Slot **out, size_t rows = 0)
{
    UCHK(get_slot(ctx, slot, out));
    Slot &s = **out;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (4 * rows > s.res_rows.cap) {
        HIPCHK(ctx, hipStreamSynchronize(s.st));  // (an earlier residual may still read the buffer being replaced)
        UCHK(s.res_rows.grow(ctx, 4 * rows));
    }
    return UGSM_OK;
}

template <class F>
int timed_launch(ugsm_ctx *ctx, Slot *s, int slot, double pixels, F &&launch)
{
    {
        Timer t(ctx, s, slot, KC_MISC, pixels);
        launch();
    }
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

int warp(ugsm_ctx *ctx, int slot, const WarpArgs &a, int in)
{
    Slot *s;
    UCHK(warp_begin(ctx, slot, &s));
    return timed_launch(ctx, s, slot, (double)a.planes * a.W * a.H, [&] { launch_warp(s->st, a, in); });
}

int residual(ugsm_ctx *ctx, int slot, ResidualArgs &a, int in, double *sums)
{
    Slot *s;
    UCHK(warp_begin(ctx, slot, &s, (size_t)a.levels * a.H));
    a.rowsum = s->res_rows;
    return timed_launch(ctx, s, slot, (double)a.levels * a.W * a.H, [&] { launch_residual(s->st, a, in, sums); });
}

}  // namespace

extern "C" {

int ugsm_warp_planes(ugsm_ctx *ctx, int slot, const float *d_src, int channels, int W, int H, const float *d_dispx, const float *d_dispy,
                     float *d_dst)
{
    if (!ctx || !d_src || !d_dispx || !d_dispy || !d_dst || d_dst == d_src || !shape_ok(W, H) || channels < 1 || channels > kMaxWarpPlanes)
        return UGSM_ERR_BAD_ARG;
    return warp(ctx, slot, WarpArgs{d_src, 0, W, H, channels, channels, d_dispx, d_dispy, d_dst}, kInPlanes);
}

int ugsm_warp_right(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbR, int W, int H, int stride, const float *d_dispx, const float *d_dispy,
                    float *d_warp3)
{
    if (!ctx || !d_rgbR || !d_dispx || !d_dispy || !d_warp3 || !shape_ok(W, H) || input_status(ctx, W, stride, d_rgbR) != UGSM_OK) return UGSM_ERR_BAD_ARG;
    return warp(ctx, slot, WarpArgs{d_rgbR, stride, W, H, 3, 3, d_dispx, d_dispy, d_warp3}, ctx->hooks.input_format);
}

int ugsm_warp_right_fovea(ugsm_ctx *ctx, int slot, const float *d_pyrR, const float *d_stackx, const float *d_stacky, int fovW, int fovH,
                          float *d_warp)
{
    if (!ctx || !d_pyrR || !d_stackx || !d_stacky || !d_warp || d_warp == d_pyrR || !shape_ok(fovW, fovH) || ctx->cfg.fovea_levels < 2)
        return UGSM_ERR_BAD_ARG;
    return warp(ctx, slot, WarpArgs{d_pyrR, 0, fovW, fovH, 3 * ctx->cfg.fovea_levels, 3, d_stackx, d_stacky, d_warp}, kInPlanes);
}

int ugsm_photometric_residual(ugsm_ctx *ctx, int slot, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride,
                              const float *d_dispx, const float *d_dispy, const float *d_conf, double *d_sums4)
{
    if (!ctx || !d_rgbL || !d_rgbR || !d_dispx || !d_dispy || !d_sums4 || ((uintptr_t)d_sums4 & 7) || !shape_ok(W, H) ||
        input_status(ctx, W, stride, d_rgbL, d_rgbR) != UGSM_OK)
        return UGSM_ERR_BAD_ARG;
    ResidualArgs a{d_rgbL, d_rgbR, stride, W, H, 1, d_dispx, d_dispy, d_conf, nullptr};
    return residual(ctx, slot, a, ctx->hooks.input_format, d_sums4);
}

int ugsm_photometric_residual_fovea(ugsm_ctx *ctx, int slot, const float *d_pyrL, const float *d_pyrR, const float *d_stackx,
                                    const float *d_stacky, const float *d_stackc, int fovW, int fovH, double *d_sums)
{
    if (!ctx || !d_pyrL || !d_pyrR || !d_stackx || !d_stacky || !d_sums || ((uintptr_t)d_sums & 7) || !shape_ok(fovW, fovH) ||
        ctx->cfg.fovea_levels < 2)
        return UGSM_ERR_BAD_ARG;
    ResidualArgs a{d_pyrL, d_pyrR, 0, fovW, fovH, ctx->cfg.fovea_levels, d_stackx, d_stacky, d_stackc, nullptr};
    return residual(ctx, slot, a, kInPlanes, d_sums);
}

}  // extern "C"
