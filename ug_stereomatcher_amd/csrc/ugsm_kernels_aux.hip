// ugsm_kernels_aux.hip -- the plain per-pixel kernels the match itself needs around the matcher proper.
//
// k_seed (a level's starting field where the next level's K-cost does not seed itself), k_copy_view (the fovea / pyramid stacks),
// k_lr_check (the opt-in LR-consistency check, on a field and on a stack), k_rgb_planes (level 0 of a pyramid of fewer than three levels:
// BASELINE configs[0]), k_level0_windows (level 0 inside the windows of a multi-window foveated call), k_wdiff_rows / k_wdiff_total
// (SURVEY 8f row f-4).  All HBM- or launch-bound.  Fields between levels and stacks: ugsm_kernels_fields.hip; the X, Y, Z planes and
// the depth images: ugsm_kernels_depth.hip; the point clouds: ugsm_kernels_cloud.hip; the warp and the photometric residual: ugsm_kernels_warp.hip.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#include "ugsm_device.hpp"
#include "ugsm_launch.hpp"

namespace ugsm {

// --------------------------------------------------------------------------------------
// MatchLib.cu:372-401 (+ fovea crop MatchGPULib.cpp:1642-1644):
// dst[x,y] = f32(SCALE * src[floor((x+cx+.5f)*sf), floor((y+cy+.5f)*sf)]), sf=(float)(1/SCALE)
// (batched: blockIdx.z = 3 x pair + plane)
__global__ void k_seed(const float *__restrict__ src3, int Ws, int Hs, float *__restrict__ dst3, int Wd, int Hd, int cx, int cy, Batch bt)
{
    int ix = blockIdx.x * blockDim.x + threadIdx.x;
    int iy = blockIdx.y;
    int plane = blockIdx.z;
    if (bt.n > 1) {
        const int b = plane / 3;
        plane -= 3 * b;
        src3 = shifted(src3, bt.in[b]);
        dst3 = shifted(dst3, bt.out[b]);
        cx = bt.cx[b];
        cy = bt.cy[b];
    }
    if (ix >= Wd) return;
    const float sf = (float)(1 / UGSM_SCALE);
    int sx = tex_index(((float)(ix + cx) + 0.5f) * sf, Ws);
    int sy = tex_index(((float)(iy + cy) + 0.5f) * sf, Hs);
    float v = src3[(size_t)plane * Ws * Hs + (size_t)sy * Ws + sx];
    dst3[(size_t)plane * Wd * Hd + (size_t)iy * Wd + ix] = (float)(UGSM_SCALE * (double)v);
}

// fovea-stack / pyramid-stack packing: plain 2-D crop copy of 3 planes
// (batched: blockIdx.z = 3 x pair + plane)
__global__ void k_copy_view(Img3 src, int W, int H, float *__restrict__ dst, size_t dst_plane, int dst_pitch, Batch bt)
{
    int ix = blockIdx.x * blockDim.x + threadIdx.x;
    int iy = blockIdx.y;
    int plane = blockIdx.z;
    if (bt.n > 1) {
        const int b = plane / 3;
        plane -= 3 * b;
        src.p = shifted(src.p, bt.img[b]);
        dst = shifted(dst, bt.out[b]);
    }
    if (ix >= W) return;
    dst[(size_t)plane * dst_plane + (size_t)iy * dst_pitch + ix] = src.p[(size_t)plane * src.plane + (size_t)iy * src.pitch + ix];
}

void launch_seed(hipStream_t st, const float *src3, int Ws, int Hs, float *dst3, int Wd, int Hd, int cx, int cy, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    UGSM_LAUNCH(k_seed, grid2(Wd, Hd, 3 * (B.n > 1 ? B.n : 1)), dim3(256), 0, st, src3, Ws, Hs, dst3, Wd, Hd, cx, cy, B);
}
void launch_copy_view(hipStream_t st, Img3 src, int W, int H, float *dst, size_t dst_plane, int dst_pitch, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    UGSM_LAUNCH(k_copy_view, grid2(W, H, 3 * (B.n > 1 ? B.n : 1)), dim3(256), 0, st, src, W, H, dst, dst_plane, dst_pitch, B);
}
// --------------------------------------------------------------------------------------
// LR-consistency check (BASELINE.json north_star; the reference has none: SURVEY.md 0.4 -- the build's own definition, DESIGN.md
// section 8; opt-in, off in every parity run).  left3 / right3: (dx, dy, conf) of the left-to-right match and of the match with the
// images exchanged.  Left pixel (x, y) matches right pixel (x + dx, y + dy) (getPointCloud.cpp:910-913); the right field is fetched
// there as the matcher fetches (tex_index on the warp's float coordinate, MatchLib.cu:510-515) and must point back within tau in x
// and in y, or the left confidence becomes 0.  `marked` (may be null) counts the pixels.  One pass: 12 B read + gather, 4 B written.
__global__ __launch_bounds__(256) void k_lr_check(float *__restrict__ left3, const float *__restrict__ right3, int W, int H, float tau,
                                                  unsigned long long *__restrict__ marked)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y;
    bool bad = false;
    if (ix < W) {
        const size_t n = (size_t)W * H, at = (size_t)iy * W + ix;
        const float dxl = left3[at], dyl = left3[n + at];
        const int sx = tex_index(((float)ix + 0.5f) + dxl, W), sy = tex_index(((float)iy + 0.5f) + dyl, H);
        const size_t rt = (size_t)sy * W + sx;
        const float ex = fabsf(dxl + right3[rt]), ey = fabsf(dyl + right3[n + rt]);
        bad = !(ex <= tau) || !(ey <= tau);
        if (bad) left3[2 * n + at] = 0.0f;
    }
    if (marked) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(bad);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(marked, (unsigned long long)__builtin_popcountll(m));
    }
}
void launch_lr_check(hipStream_t st, float *left3, const float *right3, int W, int H, float tau, unsigned long long *marked)
{
    UGSM_LAUNCH(k_lr_check, grid2(W, H), dim3(256), 0, st, left3, right3, W, H, tau, marked);
}
// The stack form: the same rule on every level of the fovea stacks of ls.n pairs (LrStack, ugsm_launch.hpp), blockIdx.z = pair x F + level.
// The two stacks of a pair have one layout, so a level's dx, dy and conf planes lie F, 2 F levels apart in either.  One count word per
// (pair, level): whole numbers, so the order of the waves' additions never shows.
// With F = 1 a "stack" is one full-frame field (3 planes of W x H), which is how a checked full-mode call (ugsm_submit_full_checked) checks BOTH
// directions of its pairs in one launch: entry 2 b is pair b's left-to-right field against its right-to-left one, entry 2 b + 1 the same two
// exchanged.  That is race-free: a thread reads dx and dy of its own field and of the other one -- planes no thread of the launch writes --
// and writes only its own field's confidence plane, which no thread reads; so each check sees the other direction's UNCHECKED dx and dy
// whatever order the workgroups run in, and no byte written through stack0 is read through back0 (the __restrict__ pair holds).
__global__ __launch_bounds__(256) void k_lr_check(float *__restrict__ stack0, const float *__restrict__ back0, int fovW, int fovH, float tau,
                                                  unsigned long long *__restrict__ marked, LrStack ls)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y;
    const int b = blockIdx.z / ls.F, k = blockIdx.z - b * ls.F;
    const size_t n = (size_t)fovW * fovH, pl = (size_t)ls.F * n;  // a level's plane; a plane of the stack
    float *const fwd = shifted(stack0, ls.fwd[b]) + (size_t)k * n;
    const float *const back = shifted(back0, ls.back[b]) + (size_t)k * n;
    bool bad = false;
    if (ix < fovW) {
        const size_t at = (size_t)iy * fovW + ix;
        const float dxl = fwd[at], dyl = fwd[pl + at];
        const int sx = tex_index(((float)ix + 0.5f) + dxl, fovW), sy = tex_index(((float)iy + 0.5f) + dyl, fovH);
        const size_t rt = (size_t)sy * fovW + sx;
        const float ex = fabsf(dxl + back[rt]), ey = fabsf(dyl + back[pl + rt]);
        bad = !(ex <= tau) || !(ey <= tau);
        if (bad) fwd[2 * pl + at] = 0.0f;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(marked + blockIdx.z, (unsigned long long)__builtin_popcountll(m));
}
void launch_lr_check(hipStream_t st, float *stack0, const float *back0, int fovW, int fovH, float tau, unsigned long long *marked, const LrStack &ls)
{
    UGSM_LAUNCH(k_lr_check, grid2(fovW, fovH, ls.n * ls.F), dim3(256), 0, st, stack0, back0, fovW, fovH, tau, marked, ls);
}

// --------------------------------------------------------------------------------------
// MatchGPULib.cpp:332-338 : rgb8 interleaved -> 3 planar f32; every input layout (InLayout, ugsm_device.hpp) an instance, each pixel read
// as its conversion to rgb8 reads
template <int L>
__global__ void k_rgb_planes(const uint8_t *__restrict__ rgb, int stride, int W, int H, float *__restrict__ planes)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    if (x >= W) return;
    float f[3];
    InPix<L>::loadf(rgb + (size_t)y * stride + InPix<L>::bpp * x, f);
    size_t n = (size_t)W * H, at = (size_t)y * W + x;
    planes[at] = f[0];
    planes[n + at] = f[InPix<L>::mono ? 0 : 1];
    planes[2 * n + at] = f[InPix<L>::mono ? 0 : 2];
}

void launch_rgb_planes(hipStream_t st, const uint8_t *rgb, int stride, int W, int H, float *planes, int fmt)
{
    with_layout(input_layout(fmt, input_words_aligned(rgb, stride, nullptr)), [&](auto layout) {
        UGSM_LAUNCH(k_rgb_planes<decltype(layout)::value>, grid2(W, H), dim3(256), 0, st, rgb, stride, W, H, planes);
    });
}

// Level 0 inside the windows (ugsm_submit_foveated_multi): level 0 of BOTH images of one pair, inside the win.n
// fovea windows (Level0Windows, ugsm_launch.hpp) and nowhere else -- the pyramid pass of such a call stores no level 0 (kPyrNoLevel0).
// blockIdx.z = 2 x window + image side; a thread converts one pixel as above.  Overlapping windows write equal values: no ordering.
template <int L>
__global__ void k_level0_windows(const uint8_t *__restrict__ rgbL, const uint8_t *__restrict__ rgbR, int stride, int W, int H, float *__restrict__ planesL,
                                 float *__restrict__ planesR, Level0Windows win)
{
    const int k = blockIdx.z >> 1, side = blockIdx.z & 1;
    const int fx = blockIdx.x * blockDim.x + threadIdx.x;
    const int x = win.x0[k] + fx, y = win.y0[k] + (int)blockIdx.y;
    if (fx >= win.w || x >= W || y >= H) return;  // (the windows lie inside the frame: fovea_geometry; the launcher refuses others)
    const uint8_t *const rgb = side ? rgbR : rgbL;
    float *const planes = side ? planesR : planesL;
    float f[3];
    InPix<L>::loadf(rgb + (size_t)y * stride + InPix<L>::bpp * x, f);
    const size_t n = (size_t)W * H, at = (size_t)y * W + x;
    planes[at] = f[0];
    planes[n + at] = f[InPix<L>::mono ? 0 : 1];
    planes[2 * n + at] = f[InPix<L>::mono ? 0 : 2];
}

bool launch_level0_windows(hipStream_t st, const uint8_t *rgbL, const uint8_t *rgbR, int stride, int W, int H, float *planesL, float *planesR,
                           const Level0Windows &win, int fmt)
{
    if (win.n < 1 || win.n > kMaxBatch || win.w < 1 || win.h < 1) return false;
    for (int k = 0; k < win.n; k++)
        if (win.x0[k] < 0 || win.y0[k] < 0 || win.x0[k] + win.w > W || win.y0[k] + win.h > H) return false;
    const bool words = input_words_aligned(rgbL, stride, nullptr) && input_words_aligned(rgbR, stride, nullptr);
    with_layout(input_layout(fmt, words), [&](auto layout) {
        UGSM_LAUNCH(k_level0_windows<decltype(layout)::value>, grid2(win.w, win.h, 2 * win.n), dim3(256), 0, st, rgbL, rgbR, stride, W, H, planesL, planesR, win);
    });
    return true;
}

// =========================================================================================
// the convergence measure of the reference's (never called) early exit -- weightedDifference,
// MatchGPULib.cpp:1336-1437 with kernels 17 / 18 (MatchLib.cu:1174-1373): sum(|D - OldD| * conf) / sum(conf) for dx and dy.
// The reference's reduction has no defined order (and is called with the block count as the block size); this build's
// definition (the CPU restatement used by the tests mirrors it) is a fixed order of binary64 sums that maps onto one wave per
// row: lane l adds its columns x = l (mod 64) left to right, lane 0 adds the 64 lane sums in lane order; a second, single-wave
// kernel adds the rows the same way.  Deterministic, and bit-identical to the CPU restatement.
// =========================================================================================
__global__ __launch_bounds__(64) void k_wdiff_rows(const float *__restrict__ newd3, const float *__restrict__ oldd3, int W, int H,
                                                  double *__restrict__ rowsum)
{
    __shared__ double sp[3][64];
    const int y = blockIdx.x, l = threadIdx.x;
    const size_t n = (size_t)W * H;
    double ph = 0.0, pv = 0.0, pc = 0.0;
    for (int x = l; x < W; x += 64) {
        const size_t at = (size_t)y * W + x;
        const float c = newd3[2 * n + at];
        float th = fabsf(newd3[at] - oldd3[at]);        // kernel 17, MatchLib.cu:1194-1199: abs(a - b) ...
        float tv = fabsf(newd3[n + at] - oldd3[n + at]);
        th = th * c;                                    // ... times conf, in float
        tv = tv * c;
        ph += (double)th;
        pv += (double)tv;
        pc += (double)c;
    }
    sp[0][l] = ph;
    sp[1][l] = pv;
    sp[2][l] = pc;
    __syncthreads();
    if (l < 3) {
        double r = 0.0;
        for (int i = 0; i < 64; i++) r += sp[l][i];
        rowsum[(size_t)y * 3 + l] = r;
    }
}
__global__ __launch_bounds__(64) void k_wdiff_total(const double *__restrict__ rowsum, int H, double *__restrict__ out3)
{
    __shared__ double sp[3][64];
    const int l = threadIdx.x;
    double p[3] = {0.0, 0.0, 0.0};
    for (int y = l; y < H; y += 64)
        for (int k = 0; k < 3; k++) p[k] += rowsum[(size_t)y * 3 + k];
    for (int k = 0; k < 3; k++) sp[k][l] = p[k];
    __syncthreads();
    if (l < 3) {
        double r = 0.0;
        for (int i = 0; i < 64; i++) r += sp[l][i];
        out3[l] = r;
    }
}
// out3 (device): S_dx, S_dy, C; rowsum: 3 * H doubles of scratch
void launch_weighted_difference(hipStream_t st, const float *newd3, const float *oldd3, int W, int H, double *rowsum, double *out3)
{
    UGSM_LAUNCH(k_wdiff_rows, dim3(H), dim3(64), 0, st, newd3, oldd3, W, H, rowsum);
    UGSM_LAUNCH(k_wdiff_total, dim3(1), dim3(64), 0, st, (const double *)rowsum, H, out3);
}

}  // namespace ugsm
