// ugsm_kernels_aux.hip -- the plain per-pixel kernels around the matcher proper.
//
// k_seed (a level's starting field where the next level's K-cost does not seed itself; its restriction form: a level's starting field from a
// full-resolution prior, the seeded full-mode call), k_copy_view (the fovea / pyramid stacks; its prolongation form: a level's field at
// full resolution in one launch, the coarse half of a full-mode call),
// k_rgb_planes (level 0 of a pyramid of fewer than three levels: BASELINE configs[0]; its window form: level 0 inside the windows of a
// multi-window foveated call), k_lr_check (the opt-in LR-consistency check),
// k_triangulate[_fovea] (the X, Y, Z planes and, as other forms of the same kernels, the coloured point cloud),
// k_upsample_paste (row f-3; its form over the stacks of several windows; and its pointwise form: the starting fields of a warm foveated
// call from a prior stack), k_wdiff_* (row f-4; and, as other forms, the photometric residual of a match), the warp form of k_rgb_planes (MatchGPULib::warpRightImage).  All HBM- or launch-bound.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#include "ugsm_device.hpp"
#include "ugsm_launch.hpp"

namespace ugsm {

static inline dim3 grid2(int W, int H, int z = 1) { return dim3((W + 255) / 256, H, z); }

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

// The restriction form (k_restrict in the statistics; ugsm_submit_full_seeded -- no reference counterpart): level s's
// starting field (rm.w x rm.h) from a full-resolution field (rm.W x rm.H, planes dx, dy, conf), read at the sites the image pyramid itself
// samples level s's pixels from.  k = s / 2.  Even s: k steps of the pyramid's sf = 2.0f sampling, tex_index((c + .5f) * 2) -- column x reads
// column ((x + 1) << k) - 1 of level 0; the closed form carries the first k - 1 steps, the last one keeps its tex_index.  Odd s: the same k
// steps down to level 1, c1 = ((x + 1) << k) - 1, then level 1's own site in level 0, tex_index((c1 + .5f) * (float)SCALE).  Rows likewise:
// the source row is one scalar per workgroup.
// Values: dx and dy of an odd level are q = f32((double)v / SCALE), the partner of k_seed's f32(SCALE * (double)v), then q * 2^-k; of an even
// level v * 2^-k (rm.scale = 2^-k, exact in binary32); the confidence is copied.  s = 0: a copy.
// (batched: blockIdx.z = 3 x pair + plane; pair b's full-resolution field at src3 + bt.in[b] bytes)
__device__ __forceinline__ int restrict_site(const int c, const int k, const int odd, const int n)
{
    if (odd) return tex_index(((float)(((c + 1) << k) - 1) + 0.5f) * (float)UGSM_SCALE, n);
    if (k == 0) return c < n ? c : n - 1;
    return tex_index(((float)(((c + 1) << (k - 1)) - 1) + 0.5f) * 2.0f, n);
}
__global__ void k_seed(const float *__restrict__ src3, RestrictMap rm, float *__restrict__ dst3, Batch bt)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    int plane = blockIdx.z;
    if (bt.n > 1) {
        const int b = plane / 3;
        plane -= 3 * b;
        src3 = shifted(src3, bt.in[b]);
        dst3 = shifted(dst3, bt.out[b]);
    }
    if (ix >= rm.w) return;
    const int sy = restrict_site(iy, rm.k, rm.odd, rm.H);
    const int sx = restrict_site(ix, rm.k, rm.odd, rm.W);
    float v = src3[(size_t)plane * rm.W * rm.H + (size_t)sy * rm.W + sx];
    if (plane < 2) {
        if (rm.odd) v = (float)((double)v / UGSM_SCALE);
        if (rm.k) v = v * rm.scale;
    }
    dst3[(size_t)plane * rm.w * rm.h + (size_t)iy * rm.w + ix] = v;
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

// The prolongation form (k_prolong in the statistics; ugsm_submit_full_coarse, ugsm_stage_prolong -- DESIGN.md section 8): the field of level
// e (pm.ws x pm.hs) at full resolution (pm.W x pm.H), pointwise.  By definition e steps of k_seed, P_l = k_seed(P_l+1) for l = e-1 .. 0 with
// no crop; here P_1 .. P_e-1 are never formed: an output pixel walks its column down through the sizes w[1 .. e] -- tex_index(((float)c +
// 0.5f) * sf, w[l]) at every level, whose clamp binds at some levels and not at others, so no closed form --, its row likewise (one site per
// workgroup: blockIdx.y alone decides it), gathers the three planes' values there and multiplies each e times by SCALE in binary64, every
// product rounded to binary32 on its own as the chain rounds it.  e = 0: a copy of a view, like the form above.
// One thread does the three planes of four pixels, in 4 / V pieces of V consecutive pixels (V = pm.vec: 4, 2 or 1 -- what the rows'
// alignment allows, prolong_vec), piece c of a workgroup's 1024 columns at (c * 256 + thread) * V: every store instruction of a wave covers
// consecutive bytes, 16 per lane where V = 4.  The four columns walk down together, a level's size read once for them.  The source is read
// about 2^e times per value, from L2; the launch is bound by the 3 W H floats it writes.  No LDS, no atomics.
// (batched: blockIdx.z = pair; pair b's state at src3 + bt.in[b] bytes, its output at dst3 + bt.out[b] bytes -- moved as pointers, not
// through integers as shifted() does: the accesses stay global ones)
template <int V>
__device__ __forceinline__ void prolong_row(const float *__restrict__ srow, const size_t splane, float *__restrict__ drow, const size_t dplane, const ProlongMap &pm)
{
    struct alignas(4 * V) Vec {
        float v[V];
    };
    const float sf = (float)(1 / UGSM_SCALE);
    int x[4], sx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) sx[k] = x[k] = blockIdx.x * 1024 + ((k / V) * 256 + (int)threadIdx.x) * V + k % V;
    for (int l = 1; l <= pm.e; l++) {
        const int n = pm.w[l];
#pragma unroll
        for (int k = 0; k < 4; k++) sx[k] = tex_index(((float)sx[k] + 0.5f) * sf, n);
    }
#pragma unroll
    for (int c = 0; c < 4 / V; c++) {
        if (x[c * V] >= pm.W) return;  // (pm.W is a multiple of V: a piece lies inside the row or outside it)
        Vec o[3];
#pragma unroll
        for (int j = 0; j < V; j++) {
#pragma unroll
            for (int p = 0; p < 3; p++) {
                float v = srow[p * splane + sx[c * V + j]];
                for (int l = 0; l < pm.e; l++) v = (float)(UGSM_SCALE * (double)v);
                o[p].v[j] = v;
            }
        }
#pragma unroll
        for (int p = 0; p < 3; p++) *reinterpret_cast<Vec *>(drow + p * dplane + x[c * V]) = o[p];
    }
}
__global__ __launch_bounds__(256) void k_copy_view(const float *__restrict__ src3, ProlongMap pm, float *__restrict__ dst3, Batch bt)
{
    if (bt.n > 1) {
        src3 = reinterpret_cast<const float *>(reinterpret_cast<const char *>(src3) + bt.in[blockIdx.z]);
        dst3 = reinterpret_cast<float *>(reinterpret_cast<char *>(dst3) + bt.out[blockIdx.z]);
    }
    const float sf = (float)(1 / UGSM_SCALE);
    const int iy = blockIdx.y;
    int sy = iy;
    for (int l = 1; l <= pm.e; l++) sy = tex_index(((float)sy + 0.5f) * sf, pm.h[l]);
    const size_t splane = (size_t)pm.ws * pm.hs, dplane = (size_t)pm.W * pm.H;
    const float *srow = src3 + (size_t)sy * pm.ws;
    float *drow = dst3 + (size_t)iy * pm.W;
    if (pm.vec == 4) prolong_row<4>(srow, splane, drow, dplane, pm);
    else if (pm.vec == 2) prolong_row<2>(srow, splane, drow, dplane, pm);
    else prolong_row<1>(srow, splane, drow, dplane, pm);
}

void launch_seed(hipStream_t st, const float *src3, int Ws, int Hs, float *dst3, int Wd, int Hd, int cx, int cy, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    UGSM_LAUNCH(k_seed, grid2(Wd, Hd, 3 * (B.n > 1 ? B.n : 1)), dim3(256), 0, st, src3, Ws, Hs, dst3, Wd, Hd, cx, cy, B);
}
void launch_restrict(hipStream_t st, const float *src3, int W, int H, int level, float *dst3, int w, int h, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    const int k = level / 2;
    const RestrictMap rm{W, H, w, h, k, level & 1, 1.0f / (float)(1 << k)};
    UGSM_LAUNCH(k_seed, grid2(w, h, 3 * (B.n > 1 ? B.n : 1)), dim3(256), 0, st, src3, rm, dst3, B);
}
void launch_copy_view(hipStream_t st, Img3 src, int W, int H, float *dst, size_t dst_plane, int dst_pitch, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    UGSM_LAUNCH(k_copy_view, grid2(W, H, 3 * (B.n > 1 ? B.n : 1)), dim3(256), 0, st, src, W, H, dst, dst_plane, dst_pitch, B);
}
// the widest store every row of every plane of every pair's output is aligned for: 16 bytes, 8, or 4
static int prolong_vec(const float *dst3, int W, const Batch &B)
{
    for (int v = 4; v > 1; v >>= 1) {
        bool ok = W % v == 0 && reinterpret_cast<uintptr_t>(dst3) % (4 * v) == 0;
        for (int b = 0; ok && b < B.n; b++) ok = B.out[b] % (4 * v) == 0;
        if (ok) return v;
    }
    return 1;
}
bool launch_prolong(hipStream_t st, const float *src3, const int *w, const int *h, int level, float *dst3, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    if (level < 0 || level >= kProlongMaxLevels || B.n > kMaxBatch || w[0] < 1 || h[0] < 1 || h[0] > 65535) return false;
    ProlongMap pm{};
    pm.W = w[0];
    pm.H = h[0];
    pm.ws = w[level];
    pm.hs = h[level];
    pm.e = level;
    pm.vec = prolong_vec(dst3, w[0], B);
    for (int l = 0; l <= level; l++) {
        if (w[l] < 1 || h[l] < 1) return false;  // (tex_index clamps to n - 1: every read lies inside its level)
        pm.w[l] = w[l];
        pm.h[l] = h[l];
    }
    UGSM_LAUNCH(k_copy_view, dim3((w[0] + 1023) / 1024, h[0], B.n > 1 ? B.n : 1), dim3(256), 0, st, src3, pm, dst3, B);
    return true;
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

// The window form (k_level0_windows in the statistics; ugsm_submit_foveated_multi): level 0 of BOTH images of one pair, inside the win.n
// fovea windows (Level0Windows, ugsm_launch.hpp) and nowhere else -- the pyramid pass of such a call stores no level 0 (kPyrNoLevel0).
// blockIdx.z = 2 x window + image side; a thread converts one pixel as above.  Overlapping windows write equal values: no ordering.
template <int L>
__global__ void k_rgb_planes(const uint8_t *__restrict__ rgbL, const uint8_t *__restrict__ rgbR, int stride, int W, int H, float *__restrict__ planesL,
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
    using Kern = void (*)(const uint8_t *, const uint8_t *, int, int, int, float *, float *, Level0Windows);
    with_layout(input_layout(fmt, words), [&](auto layout) {
        const Kern kern = k_rgb_planes<decltype(layout)::value>;
        UGSM_LAUNCH(kern, grid2(win.w, win.h, 2 * win.n), dim3(256), 0, st, rgbL, rgbR, stride, W, H, planesL, planesR, win);
    });
    return true;
}

// The warp form (ugsm_warp_planes, ugsm_warp_right, ugsm_warp_right_fovea): MatchGPULib::warpRightImage, MatchGPULib.cpp:1445-1518 over kernel
// warpAbyB (MatchLib.cu:499-549) -- dst[iy][ix] = src[tex(iy + .5f + dy)][tex(ix + .5f + dx)], K-cost's own fetch (ugsm_kernels_march.hip),
// the value stored as it was fetched.  One template over the source (WarpArgs, ugsm_launch.hpp): kInPlanes -- float planes in, blockIdx.z the
// plane, warped by field z / per_field (one field for every plane, or a fovea stack's level = z / 3); an InLayout -- the 8-bit image in, the
// gathered pixel read once for its three planes.  HBM-bound: 8 B of (dx, dy), one gathered value, 4 (12) B written per thread.
template <int L>
__global__ __launch_bounds__(256) void k_rgb_planes(WarpArgs a)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y;
    if (ix >= a.W) return;
    const size_t n = (size_t)a.W * a.H, at = (size_t)iy * a.W + ix;
    const size_t field = L == kInPlanes ? (size_t)((int)blockIdx.z / a.per_field) * n : 0;
    const int sx = tex_index(((float)ix + 0.5f) + a.dx[field + at], a.W);
    const int sy = tex_index(((float)iy + 0.5f) + a.dy[field + at], a.H);
    if constexpr (L == kInPlanes) {
        const size_t pl = (size_t)blockIdx.z * n;
        a.dst[pl + at] = static_cast<const float *>(a.src)[pl + (size_t)sy * a.W + sx];
    } else {
        float f[3];
        InPix<L>::loadf(static_cast<const uint8_t *>(a.src) + (size_t)sy * a.stride + InPix<L>::bpp * sx, f);
        a.dst[at] = f[0];
        a.dst[n + at] = f[InPix<L>::mono ? 0 : 1];
        a.dst[2 * n + at] = f[InPix<L>::mono ? 0 : 2];
    }
}

void launch_warp(hipStream_t st, const WarpArgs &a, int in)
{
    using Kern = void (*)(WarpArgs);
    if (in == kInPlanes) {
        const Kern kern = k_rgb_planes<kInPlanes>;
        UGSM_LAUNCH(kern, grid2(a.W, a.H, a.planes), dim3(256), 0, st, a);
        return;
    }
    const bool words = input_words_aligned(static_cast<const uint8_t *>(a.src), a.stride, nullptr);
    with_layout(input_layout(in, words), [&](auto layout) {
        const Kern kern = k_rgb_planes<decltype(layout)::value>;
        UGSM_LAUNCH(kern, grid2(a.W, a.H), dim3(256), 0, st, a);
    });
}

// =========================================================================================
// triangulation of the full-resolution disparity into X, Y, Z planes.
// CdynamicCalibration::get3DPoint, non-foveated branch (src/pointcloud/getPointCloud.cpp:886-949), for
// every pixel: the reference calls it from scalar host loops behind a progress bar (:640-660, :778).
// Purely per-pixel (reads 8 B, writes 12 B): HBM-bound.  The closed form keeps the source's mix of float
// and double term by term (a..j, x, y are floats; pow(v,2.0) is the exact binary64 square; the literal
// 2.0 is a double) -- the expression text is kept identical to the CPU restatement used by the tests, no contraction.
// =========================================================================================
struct Proj {
    double m[12];  // 3x4, row major
};
__device__ __forceinline__ double sq_d(float v) { return (double)v * (double)v; }

// the closed form of get3DPoint (getPointCloud.cpp:908-948) for one left/right correspondence.
// NOTE: this one function follows the reference's expressions term for term, including its variable names
// a..j, x, y -- the formula is a machine-generated closed form whose evaluation order and float/double mix ARE the bit-exactness
// contract (re-associating any term changes the result), so the similarity is unavoidable here and deliberately confined to this
// block; nothing else in the product is written against the reference's text.
__device__ __forceinline__ void tri_point(float x1, float y1, float x2, float y2, const double *P1, const double *P2, float &X, float &Y, float &Z)
{
    float a, b, c, d, e, f, g, h, i, j, x, y;
    a = (float)P1[0];
    b = (float)(P1[2] - x1);
    c = (float)P1[5];
    d = (float)(P1[6] - y1);
    e = (float)(P2[0] - x2 * P2[8]);
    f = (float)(P2[1] - x2 * P2[9]);
    g = (float)(P2[2] - x2 * P2[10]);
    h = (float)(P2[4] - y2 * P2[8]);
    i = (float)(P2[5] - y2 * P2[9]);
    j = (float)(P2[6] - y2 * P2[10]);
    x = (float)(x2 * P2[11] - P2[3]);
    y = (float)(y2 * P2[11] - P2[7]);
    float XUp = (d*f*h - c*g*h - d*e*i + c*e*j)*(-(d*i*x) + c*j*x + d*f*y - c*g*y) +
                sq_d(b)*((f*h - e*i)*(-(i*x) + f*y) + sq_d(c)*(e*x + h*y)) +
                a*b*((-(g*i) + f*j)*(i*x - f*y) + c*d*(f*x + i*y) - sq_d(c)*(g*x + j*y));
    float YUp = (sq_d(b)*(f*h - e*i) + d*(d*f*h - c*g*h - d*e*i + c*e*j))*(h*x - e*y) +
                a*b*((c*d*e + g*h*i - 2.0*f*h*j + e*i*j)*x + (c*d*h + f*g*h - 2.0*e*g*i + e*f*j)*y) +
                sq_d(a)*((g*i - f*j)*(-(j*x) + g*y) + sq_d(d)*(f*x + i*y) - c*d*(g*x + j*y));
    float ZUp = c*(-(d*f*h) + c*g*h + d*e*i - c*e*j)*(h*x - e*y) - a*b*((f*h - e*i)*(-(i*x) + f*y) +
                sq_d(c)*(e*x + h*y)) + sq_d(a)*((g*i - f*j)*(i*x - f*y) - c*d*(f*x + i*y) +
                sq_d(c)*(g*x + j*y));
    float divisor = sq_d(b)*(sq_d(c)*(sq_d(e) + sq_d(h)) + sq_d(f*h - e*i)) +
                    sq_d(d*f*h - c*g*h - d*e*i + c*e*j) - 2.0*a*b*(-(c*d*(e*f + h*i)) +
                    (f*h - e*i)*(-(g*i) + f*j) + sq_d(c)*(e*g + h*j)) + sq_d(a)*
                    (sq_d(d)*(sq_d(f) + sq_d(i)) + sq_d(g*i - f*j) - 2.0*c*d*(f*g + i*j) +
                    sq_d(c)*(sq_d(g) + sq_d(j)));
    X = XUp / divisor;
    Y = YUp / divisor;
    Z = ZUp / divisor;
}

// The forms of k_triangulate / k_triangulate_fovea (template parameter): the X, Y, Z planes, the two launches of the point cloud and
// the two of the resized cloud, the two of the fovea stack's merged cloud and the two of the merged cloud of several windows' stacks
// (below).  The plane form keeps its own parameter list, so its code is what it was before the cloud forms came.
enum TriForm : int {
    kTriPlanes = 0, kTriCloudCount = 1, kTriCloud = 2, kTriResizedCount = 3, kTriResized = 4, kTriStackCount = 5, kTriStack = 6,
    kTriMultiCount = 7, kTriMulti = 8
};

template <int Form>
__global__ __launch_bounds__(256) void k_triangulate(const float *__restrict__ dispx, const float *__restrict__ dispy, int W, int H, Proj P1q, Proj P2q,
                                                     float *__restrict__ xyz)
{
    static_assert(Form == kTriPlanes, "the plane form");
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    if (xx >= W) return;
    const size_t n = (size_t)W * H, at = (size_t)yy * W + xx;
    float x1, x2, y1, y2;
    x1 = xx;
    y1 = yy;
    x2 = xx + dispx[at];
    y2 = yy + dispy[at];
    float X, Y, Z;
    tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
    xyz[at] = X;
    xyz[n + at] = Y;
    xyz[2 * n + at] = Z;
}

// get3DPoint, foveated branch (getPointCloud.cpp:892-903): level src_level of the (F*fovH) x fovW stacks, pixel
// coordinates mapped into the full-resolution frame by mapXcoord / mapYcoord (:387-421).  Those take an int, so the
// right-image coordinate xx + disparity is truncated toward zero before scaling -- kept as in the reference.
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate_fovea(const float *__restrict__ stackx, const float *__restrict__ stacky, int fovW, int fovH,
                                                           int src_level, int left_margin, int upper_margin, float scale, Proj P1q, Proj P2q,
                                                           float *__restrict__ xyz)
{
    static_assert(Form == kTriPlanes, "the plane form");
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    if (xx >= fovW) return;
    const size_t n = (size_t)fovW * fovH, at = (size_t)yy * fovW + xx;
    const size_t sat = ((size_t)yy + (size_t)fovH * src_level) * fovW + xx;
    const float x1 = (float)left_margin + (float)xx * scale;
    const float y1 = (float)upper_margin + (float)yy * scale;
    const int sx = (int)(xx + stackx[sat]);
    const int sy = (int)(yy + stacky[sat]);
    const float x2 = (float)left_margin + (float)sx * scale;
    const float y2 = (float)upper_margin + (float)sy * scale;
    float X, Y, Z;
    tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
    xyz[at] = X;
    xyz[n + at] = Y;
    xyz[2 * n + at] = Z;
}

void launch_triangulate(hipStream_t st, const float *dispx, const float *dispy, int W, int H, const double *P1, const double *P2, float *xyz)
{
    Proj a, b;
    for (int k = 0; k < 12; k++) { a.m[k] = P1[k]; b.m[k] = P2[k]; }
    void (*const kern)(const float *, const float *, int, int, Proj, Proj, float *) = k_triangulate<kTriPlanes>;
    UGSM_LAUNCH(kern, dim3((W + 255) / 256, H), dim3(256), 0, st, dispx, dispy, W, H, a, b, xyz);
}

void launch_triangulate_fovea(hipStream_t st, const float *stackx, const float *stacky, int fovW, int fovH, int src_level, int left_margin,
                              int upper_margin, float scale, const double *P1, const double *P2, float *xyz)
{
    Proj a, b;
    for (int k = 0; k < 12; k++) { a.m[k] = P1[k]; b.m[k] = P2[k]; }
    void (*const kern)(const float *, const float *, int, int, int, int, int, float, Proj, Proj, float *) = k_triangulate_fovea<kTriPlanes>;
    UGSM_LAUNCH(kern, dim3((fovW + 255) / 256, fovH), dim3(256), 0, st, stackx, stacky, fovW, fovH, src_level, left_margin,
                       upper_margin, scale, a, b, xyz);
}

// =========================================================================================
// SURVEY 8f row f-1, second half: the coloured point cloud, getPointCloud.cpp doReconstructionRGB (:675-722) and
// doReconstructionRGB_FOV (:615-673) -- the node's scalar double loop over the pixels with one push_back per pixel.
// Column ii is the outer loop and row jj the inner one, so the cloud is COLUMN-major while the planes are row-major: record
// (ci, cj) of the sampled grid (ii = ci * s, jj = cj * s) is record ci * hc + cj of the dense cloud.  X, Y, Z are tri_point's, from
// the same operands as the plane form computes them (bit-identical); the colour word is R << 16 | G << 8 | B of the left image
// (the node's BGR8 copy, :225, packed at :703-714), i.e. byte0 << 16 | byte1 << 8 | byte2 of the rgb8 buffer, alpha 0.
//
// One workgroup per tile of kCloudTC sampled columns x kCloudTR sampled rows, three phases:
//   A  evaluate: lane (t mod 32) = column, so every read is a row-coalesced run (4-byte dx, dy, conf; rgb bytes); the record
//      (x, y, z, rgb word) goes to LDS at [column][row] and whether it is kept to a byte array;
//   B  one wave per column, lane = row: a ballot of the kept flags gives every kept row its rank in the column's run (dense: every
//      row inside the grid is kept, so the ranks are the rows), and `src` the row of each rank;
//   C  every column's run of the tile is one contiguous block of the output, written with whole 16-byte stores, one wave instruction
//      covering 1 KB of it: 32 records of 32 B (PCL32) or 64 of 16 B (XYZRGB16).
// Compact clouds take two launches.  The count form (kTriCloudCount) runs A and B and writes each column's kept count per chunk of
// kCloudTR rows, and adds it to the column's and the strip's (the tile column's) totals with integer atomics: order-independent sums,
// deterministic.  The cloud form (kTriCloud) derives each run's first record from those counts -- the strips to its left, the strip's
// columns to its left, the chunks above it -- and re-evaluates its tile (tri_point is cheap beside a second pass over the output).
// No workgroup waits for another inside a launch.  Records at or past cap are not written; `count` gets the cloud's size.
// =========================================================================================
constexpr int kCloudTC = 32;             // sampled columns per tile
constexpr int kCloudTR = 64;             // sampled rows per tile = lanes of a wave (phase B)
constexpr int kCloudPad = kCloudTR + 1;  // records per column in LDS: column c starts 4c banks further on (phase A stores 32 columns at once)

// X, Y, Z of pixel (ii, jj) of the planes, from the same operands as the plane forms (bit-identical to them); (x1, y1) the pixel in the
// full-resolution frame.
template <bool Fovea>
__device__ __forceinline__ void tri_at(const CloudArgs &a, const Proj &P1q, const Proj &P2q, int ii, int jj, float &x1, float &y1, float &X,
                                       float &Y, float &Z)
{
    const size_t at = (size_t)jj * a.pw + ii;
    float x2, y2;
    if (Fovea) {  // as k_triangulate_fovea
        x1 = (float)a.left_margin + (float)ii * a.scale;
        y1 = (float)a.upper_margin + (float)jj * a.scale;
        const int sx = (int)(ii + a.dx[at]);
        const int sy = (int)(jj + a.dy[at]);
        x2 = (float)a.left_margin + (float)sx * a.scale;
        y2 = (float)a.upper_margin + (float)sy * a.scale;
    } else {      // as k_triangulate
        x1 = ii;
        y1 = jj;
        x2 = ii + a.dx[at];
        y2 = jj + a.dy[at];
    }
    tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
}

// The colour word of pixel cx of an image row in any input format (UGSM_INPUT_*; fmt is uniform): R << 16 | G << 8 | B of the pixel's
// conversion to rgb8.  The three- and four-byte formats read bytes 0, 1, 2 at fixed offsets (two loads) and select the channel order.
// Not a switch over the formats: that puts the colour loads and their waits ahead of the arithmetic, and the resized clouds' short
// launches take up to a sixth longer.
__device__ __forceinline__ unsigned colour_word(const uint8_t *row, int cx, int fmt)
{
    if (fmt == kInMono8) return (unsigned)row[cx] * 0x010101u;
    const bool swap = fmt == kInBGR8 || fmt == kInBGRA8;
    const uint8_t *p = row + (size_t)((fmt == kInRGBA8 || fmt == kInBGRA8) ? 4 : 3) * cx;
    const unsigned c0 = p[0], c1 = p[1], c2 = p[2];
    return (swap ? c2 : c0) << 16 | c1 << 8 | (swap ? c0 : c2);
}

// the colour word of full-resolution pixel (cx, cy); the foveated forms clamp it to the image (the reference reads whatever lies there):
// at destination level 0 no fovea level's window leaves the image at 16 MP, 1080p, 640 x 480 or 160 x 120, so the clamp only acts on
// margins a caller pushes past the edge
template <bool Clamp>
__device__ __forceinline__ unsigned colour_at(const CloudArgs &a, int cx, int cy)
{
    if (Clamp) {
        cx = min(max(cx, 0), a.W - 1);
        cy = min(max(cy, 0), a.H - 1);
    }
    return colour_word(a.rgb + (size_t)cy * a.stride, cx, a.fmt);
}

// whether a compact cloud keeps a point of pixel `at` of the planes
__device__ __forceinline__ bool cloud_keep(const CloudArgs &a, size_t at, float X, float Y, float Z)
{
    if (!a.compact) return true;
    bool keep = __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z) && Z >= a.z_min && Z <= a.z_max;
    if (a.conf) keep = keep && a.conf[at] >= a.min_conf;  // (a NaN confidence fails the comparison)
    return keep;
}

// one sampled point: its record (x, y, z, rgb word as float bits) and whether a compact cloud keeps it
template <bool Fovea, bool Colour>
__device__ __forceinline__ bool cloud_point(const CloudArgs &a, const Proj &P1q, const Proj &P2q, int ii, int jj, float4 &rec)
{
    float x1, y1, X, Y, Z;
    tri_at<Fovea>(a, P1q, P2q, ii, jj, x1, y1, X, Y, Z);
    if (Colour) {  // the foveated forms: at ((int)mapXcoord(ii), (int)mapYcoord(jj)) of the full-resolution image (:630-640), clamped (colour_at)
        const int cx = Fovea ? min(max((int)x1, 0), a.W - 1) : ii, cy = Fovea ? min(max((int)y1, 0), a.H - 1) : jj;
        rec = make_float4(X, Y, Z, __uint_as_float(colour_word(a.rgb + (size_t)cy * a.stride, cx, a.fmt)));
    }
    return cloud_keep(a, (size_t)jj * a.pw + ii, X, Y, Z);
}

// SURVEY 8f row f-1, the resized cloud: getPointCloud.cpp doReconstruction_resized (:724-800) / doReconstructionFOV_resized (:802-884),
// cv::resize(range_map, res, Size(pw * f, ph * f), 0, 0, INTER_CUBIC) of the Z plane, then one point per pixel (ii, jj) of the resized
// map, in the same column-major order.  The Z plane is never written: each point evaluates the 16 Z of its 4 x 4 footprint with tri_at
// (the plane form's Z, bit for bit) and resizes them in OpenCV's float order (resizeGeneric_ with HResizeCubic / VResizeCubic on CV_32F):
//   taps   fx = (float)((dx + 0.5) * scale_x - 0.5) with scale_x = 1. / ((double)dw / pw) in double, sx = floor(fx), fx -= sx in float;
//          columns sx-1 .. sx+2 and rows sy-1 .. sy+2 clamped to the plane (replicate border);
//   coeffs interpolateCubic, A = -0.75f, in float; c3 = 1 - c0 - c1 - c2;
//   sums   each source row ((S0*c0 + S1*c1) + S2*c2) + S3*c3 left to right, from +0.0f on the border columns (sx < 1 or sx + 2 >= pw:
//          HResizeCubic's clamped loop accumulates from 0, which only turns a -0.0f sum into +0.0f); then ((R0*b0 + R1*b1) + R2*b2) + R3*b3;
//          every product rounded on its own (the library builds with -ffp-contract=off).  NaN and inf propagate (0 * inf is NaN).
//   same   cv::resize copies the plane when the size does not change (factor 1), so there Z is the pixel's own Z.
// X, Y are get3DPoint's at xx = (int)((float)ii / f), yy = (int)((float)jj / f) (IEEE float division) -- the reference's registration:
// the cubic's centre lies near ii / f + (1 / f - 1) / 2, two pixels further on at f = 0.2, and it is kept.  The colour is the left
// image's at (xx, yy); the foveated form reads it there too, in the full image's top-left corner (:864-867), unless colour_mapped asks
// for the mapped pixel as ugsm_point_cloud_fovea reads it.  A compact cloud tests X, Y, the resized Z and conf(xx, yy).
__device__ __forceinline__ void cubic_tap(int d, double scale, int n, int &s, float c[4], bool &border)
{
    float f = (float)((d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    const float A = -0.75f;
    c[0] = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A;
    c[1] = ((A + 2) * f - (A + 3)) * f * f + 1;
    c[2] = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
    border = s < 1 || s + 2 >= n;
}

template <bool Fovea, bool Colour>
__device__ __forceinline__ bool resized_point(const CloudArgs &a, const CloudResize &rz, const Proj &P1q, const Proj &P2q, int ii, int jj,
                                              float4 &rec)
{
    // (ii < (int)(pw * f) keeps ii / f below pw; the clamp never acts)
    const int xx = min((int)((float)ii / rz.factor), a.pw - 1);
    const int yy = min((int)((float)jj / rz.factor), a.ph - 1);
    float x1, y1, X, Y, Z;
    tri_at<Fovea>(a, P1q, P2q, xx, yy, x1, y1, X, Y, Z);
    // the colour is read before the taps: its loads go out with the centre pixel's dx, dy, not one round trip after the taps
    const bool mapped = Fovea && rz.colour_mapped;
    const unsigned word = Colour ? colour_at<Fovea>(a, mapped ? (int)x1 : xx, mapped ? (int)y1 : yy) : 0u;
    if (!rz.same_size) {
        int sx, sy;
        float cx[4], cy[4];
        bool border, unused;
        cubic_tap(ii, rz.scale_x, a.pw, sx, cx, border);
        cubic_tap(jj, rz.scale_y, a.ph, sy, cy, unused);
        float v = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ty = min(max(sy - 1 + r, 0), a.ph - 1);
            float s[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float u1, u2, u3, u4;
                tri_at<Fovea>(a, P1q, P2q, min(max(sx - 1 + k, 0), a.pw - 1), ty, u1, u2, u3, u4, s[k]);
            }
            const float p0 = s[0] * cx[0];
            const float h = (((border ? 0.0f + p0 : p0) + s[1] * cx[1]) + s[2] * cx[2]) + s[3] * cx[3];
            v = r == 0 ? h * cy[0] : v + h * cy[r];
        }
        Z = v;
    }
    if (Colour) rec = make_float4(X, Y, Z, __uint_as_float(word));
    return cloud_keep(a, (size_t)yy * a.pw + xx, X, Y, Z);
}

// The merged cloud of the whole fovea stack (ugsm_point_cloud_fovea_all; kTriStackCount / kTriStack): the same tile over F * strips
// virtual strips, level = strip / strips.  `a` holds the workgroup's level already (its planes and mapping: k_triangulate_fovea, the
// overload on the table), lv is that level's row of the table.  A covered point (sampled column in [cx0, cx1) and row in [cy0, cy1): its footprint lies wholly inside
// the finer level's window) is marked not kept before any load is issued for it, so phase B ranks the rest and phase C writes them as one
// run per column; a tile wholly inside the rectangle returns at once.  Dense offsets are closed-form: the level's first record, the
// columns before this one x hc less ny for each covered one among them, the rows above less the covered ones.  Compact: the two-launch
// scheme over the F * wc virtual columns and F * strips virtual strips.
__device__ __forceinline__ long long stack_dense_run(const CloudArgs &a, const CloudLevel &lv, int ci, int r0)
{
    const int ncx = lv.cx1 - lv.cx0, ny = lv.cy1 - lv.cy0;
    const bool in = ci >= lv.cx0 && ci < lv.cx1;
    return lv.first + (long long)ci * a.hc - (long long)ny * min(max(ci - lv.cx0, 0), ncx) + r0 - (in ? min(max(r0 - lv.cy0, 0), ny) : 0);
}

// The merged cloud of several windows' stacks (ugsm_point_cloud_fovea_multi; kTriMultiCount / kTriMulti): the same tile over E * strips
// virtual strips, entry = strip / strips, E = (F-1) n + 1 entries (level-major: entry k n + j = level k of window j; the last = level F-1
// of stack 0).  What an entry leaves out is a UNION of rectangles of its sampled grid (CloudEntry), so the kernel (k_triangulate_fovea,
// the overload on CloudMulti) reduces the entry's list to what the tile needs before the tile runs, 32 lanes = the tile's columns:
//   omask[c]  the left-out rows of column c inside the tile, one bit per row: phase A marks those not kept before any load;
//   run[c]    dense: the first record of column c's run in this tile -- the entry's first record, the records of the columns before it
//             (the host's segments: between two neighbouring rectangle edges every column keeps the same number of rows) and the kept
//             rows above the tile (the row masks of the chunks above, popcounted).  No workgroup waits for another.
// Compact: the two-launch scheme over the E * wc virtual columns and E * strips virtual strips.
struct MultiTile {
    const unsigned long long *omask;
    const long long *run;
};

// bits [lo, hi) of a tile's 64 rows
__device__ __forceinline__ unsigned long long row_bits(int lo, int hi)
{
    lo = max(lo, 0);
    hi = min(hi, kCloudTR);
    if (hi <= lo) return 0ull;
    return (hi == kCloudTR ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1);
}

template <bool Fovea, int Form>
__device__ __forceinline__ void cloud_tile(const CloudArgs &a, const CloudResize &rz, const Proj &P1q, const Proj &P2q, const CloudStack *sk = nullptr,
                                           int level = 0, const CloudMulti *mu = nullptr, const MultiTile *mt = nullptr)
{
    constexpr bool Stack = Form == kTriStackCount || Form == kTriStack;
    constexpr bool Multi = Form == kTriMultiCount || Form == kTriMulti;  // (level: the entry; its early return is the kernel's)
    __shared__ float4 rec[kCloudTC * kCloudPad];
    __shared__ unsigned char kept[kCloudTC * kCloudTR];
    __shared__ unsigned char src[kCloudTC * kCloudTR];
    __shared__ int nrec[kCloudTC];
    __shared__ unsigned pre[kCloudTC + 1];  // compact: [c] the run's first record less the strip's, [kCloudTC] the strip's first record
    // tx: the strip among all of the launch (the stack forms: F * strips virtual strips); c0: its first column in its level, v0: among
    // the launch's columns (the stack forms: level * wc + c0, the F * wc virtual columns)
    const int t = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
    const int c0 = (Stack ? tx - level * sk->strips : Multi ? tx - level * ((a.wc + kCloudTC - 1) / kCloudTC) : tx) * kCloudTC, r0 = ty * kCloudTR;
    const int c = t & (kCloudTC - 1), ci = c0 + c;
    const int v0 = Stack || Multi ? level * a.wc + c0 : c0, wv = Stack ? sk->F * a.wc : Multi ? mu->E * a.wc : a.wc;
    unsigned *const col_tot = a.cnt + (size_t)wv * a.nchunk, *const strip_tot = col_tot + wv;  // (compact only)
    constexpr bool Write = Form == kTriCloud || Form == kTriResized || Form == kTriStack || Form == kTriMulti, Count = !Write;  // the cloud launch / the count launch
    if constexpr (Stack) {  // a tile wholly covered has nothing to evaluate (the workgroup that writes the size stays)
        const CloudLevel &lv = sk->lv[level];
        if (c0 >= lv.cx0 && min(c0 + kCloudTC, a.wc) <= lv.cx1 && r0 >= lv.cy0 && min(r0 + kCloudTR, a.hc) <= lv.cy1 &&
            !(ty == 0 && tx == (a.compact ? (int)gridDim.x - 1 : 0))) {
            if (Count && t < kCloudTC && c0 + t < a.wc) a.cnt[(size_t)(v0 + t) * a.nchunk + ty] = 0;
            return;
        }
    }
    if (Write && a.compact && t <= kCloudTC) pre[t] = 0;
    // A: evaluate the tile
    for (int r = t / kCloudTC; r < kCloudTR; r += 256 / kCloudTC) {
        const int cj = r0 + r;
        bool k = false;
        bool covered = false;
        if constexpr (Stack) covered = ci >= sk->lv[level].cx0 && ci < sk->lv[level].cx1 && cj >= sk->lv[level].cy0 && cj < sk->lv[level].cy1;
        if constexpr (Multi) covered = (mt->omask[c] >> r) & 1;
        if (ci < a.wc && cj < a.hc && !covered) {
            float4 v;
            if constexpr (Form == kTriResizedCount || Form == kTriResized)
                k = resized_point<Fovea, Write>(a, rz, P1q, P2q, ci, cj, v);
            else
                k = cloud_point<Fovea, Write>(a, P1q, P2q, ci * a.s, cj * a.s, v);
            if (Write) rec[c * kCloudPad + r] = v;
        }
        kept[c * kCloudTR + r] = k;
    }
    __syncthreads();
    if (Write && a.compact) {  // the runs' offsets: integer sums of the count launch's results
        unsigned v = 0, w = 0;
        for (int k = t; k < tx; k += 256) v += strip_tot[k];               // strips to the left
        if (ci < a.wc) {
            for (int k = t / kCloudTC; k < ty; k += 256 / kCloudTC) w += a.cnt[(size_t)(v0 + c) * a.nchunk + k];  // chunks above
            for (int k = t / kCloudTC; k < c; k += 256 / kCloudTC) w += col_tot[v0 + k];                          // the strip's columns to the left
        }
        if (v) atomicAdd(&pre[kCloudTC], v);
        if (w) atomicAdd(&pre[c], w);
    }
    // B: each column's kept rows, ranked
    const int lane = t & 63;
    for (int cc = t >> 6; cc < kCloudTC; cc += 4) {
        const bool k = kept[cc * kCloudTR + lane] != 0;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(k);
        if (Write && k) src[cc * kCloudTR + __builtin_popcountll(m & ((1ull << lane) - 1))] = (unsigned char)lane;
        if (lane == 0) {
            const int n = __builtin_popcountll(m);
            nrec[cc] = n;
            if (Count && c0 + cc < a.wc) {
                a.cnt[(size_t)(v0 + cc) * a.nchunk + ty] = (unsigned)n;
                if (n) {
                    atomicAdd(&col_tot[v0 + cc], (unsigned)n);
                    atomicAdd(&strip_tot[tx], (unsigned)n);
                }
            }
        }
    }
    if (Count) return;
    __syncthreads();
    // the cloud's size: one workgroup writes it
    if constexpr (Stack) {  // ... and each level's share of it: the strip totals summed per level (eight lanes a level), or the table's
        if (ty == 0 && tx == (a.compact ? (int)gridDim.x - 1 : 0)) {
            const CloudLevel &last = sk->lv[sk->F - 1];
            if (t == 0) *a.count = a.compact ? (long long)pre[kCloudTC] + strip_tot[tx] : last.first + last.points;
            if (sk->level_counts && a.compact) {
                static_assert(kCloudMaxLevels * 8 <= 256, "eight lanes per level");
                const int l = t >> 3;
                unsigned n = 0;
                if (l < sk->F)
                    for (int k = t & 7; k < sk->strips; k += 8) n += strip_tot[l * sk->strips + k];
                n += __shfl_xor(n, 1);
                n += __shfl_xor(n, 2);
                n += __shfl_xor(n, 4);
                if (l < sk->F && (t & 7) == 0) sk->level_counts[l] = (long long)n;
            } else if (sk->level_counts && t == 0) {
                for (int l = 0; l < sk->F; l++) sk->level_counts[l] = sk->lv[l].points;
            }
        }
    } else if constexpr (Multi) {  // ... and each entry's share: E may pass what eight lanes a level were sized for, so a lane loops over entries
        if (ty == 0 && tx == (a.compact ? (int)gridDim.x - 1 : 0)) {
            if (t == 0) *a.count = a.compact ? (long long)pre[kCloudTC] + strip_tot[tx] : mu->total;
            if (mu->entry_counts) {
                const int strips = (a.wc + kCloudTC - 1) / kCloudTC;
                for (int e = t; e < mu->E; e += 256) {
                    long long n = mu->table[e].points;
                    if (a.compact) {
                        n = 0;
                        for (int k = 0; k < strips; k++) n += strip_tot[e * strips + k];
                    }
                    mu->entry_counts[e] = n;
                }
            }
        }
    } else if (t == 0 && ty == 0 && tx == (a.compact ? (int)gridDim.x - 1 : 0))
        *a.count = a.compact ? (long long)pre[kCloudTC] + strip_tot[tx] : (long long)a.wc * a.hc;
    // C: every column's run, contiguous
    if (a.format == 0) {  // UGSM_CLOUD_PCL32: (x, y, z, 1.0f) and (rgb, 0, 0, 0), 32 B per record
        float4 *out = reinterpret_cast<float4 *>(a.points);
        for (int q = t; q < kCloudTC * 2 * kCloudTR; q += 256) {
            const int cc = q / (2 * kCloudTR), j = (q >> 1) & (kCloudTR - 1), half = q & 1;
            if (j >= nrec[cc]) continue;
            const long long o = (a.compact ? (long long)pre[kCloudTC] + pre[cc]
                                           : (Multi ? mt->run[cc] : Stack ? stack_dense_run(a, sk->lv[level], c0 + cc, r0) : (long long)(c0 + cc) * a.hc + r0)) + j;
            if (o >= a.cap) continue;
            const float4 v = rec[cc * kCloudPad + src[cc * kCloudTR + j]];
            out[2 * o + half] = half ? make_float4(v.w, 0.0f, 0.0f, 0.0f) : make_float4(v.x, v.y, v.z, 1.0f);
        }
    } else {              // UGSM_CLOUD_XYZRGB16: (x, y, z, rgb), 16 B per record
        float4 *out = reinterpret_cast<float4 *>(a.points);
        for (int q = t; q < kCloudTC * kCloudTR; q += 256) {
            const int cc = q / kCloudTR, j = q & (kCloudTR - 1);
            if (j >= nrec[cc]) continue;
            const long long o = (a.compact ? (long long)pre[kCloudTC] + pre[cc]
                                           : (Multi ? mt->run[cc] : Stack ? stack_dense_run(a, sk->lv[level], c0 + cc, r0) : (long long)(c0 + cc) * a.hc + r0)) + j;
            if (o >= a.cap) continue;
            out[o] = rec[cc * kCloudPad + src[cc * kCloudTR + j]];
        }
    }
}

// the cloud forms; rz: the resized forms' (unused by the others)
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate(CloudArgs a, Proj P1q, Proj P2q, CloudResize rz)
{
    static_assert(Form != kTriPlanes, "the cloud forms");
    cloud_tile<false, Form>(a, rz, P1q, P2q);
}
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate_fovea(CloudArgs a, Proj P1q, Proj P2q, CloudResize rz)
{
    static_assert(Form != kTriPlanes, "the cloud forms");
    cloud_tile<true, Form>(a, rz, P1q, P2q);
}

// the merged cloud of the fovea stack (an overload on the table): the workgroup's level from its strip, that level's planes and mapping
// into its copy of the arguments
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate_fovea(CloudArgs a, Proj P1q, Proj P2q, CloudStack sk)
{
    static_assert(Form == kTriStackCount || Form == kTriStack, "the stack forms");
    const int level = blockIdx.x / sk.strips;
    const CloudLevel &lv = sk.lv[level];
    a.dx += lv.plane;
    a.dy += lv.plane;
    if (a.conf) a.conf += lv.plane;
    a.left_margin = lv.left_margin;
    a.upper_margin = lv.upper_margin;
    a.scale = lv.scale;
    cloud_tile<true, Form>(a, CloudResize{}, P1q, P2q, &sk, level);
}

// The same forms for the pairs of a queue call in one launch (overloads on the table): blockIdx.z = the pair, whose row of the table in
// device memory is what the single-pair forms take as kernel arguments.  The tile is cloud_tile, untouched: blockIdx.x, blockIdx.y and
// gridDim.x are the single-pair launch's.
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate(const CloudPair *__restrict__ table, Proj P1q, Proj P2q)
{
    static_assert(Form == kTriCloudCount || Form == kTriCloud, "the cloud forms of a call's pairs");
    const CloudArgs a = table[blockIdx.z].a;
    cloud_tile<false, Form>(a, CloudResize{}, P1q, P2q);
}
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate_fovea(const CloudPair *__restrict__ table, Proj P1q, Proj P2q)
{
    static_assert(Form == kTriStackCount || Form == kTriStack, "the stack forms of a call's pairs");
    const CloudPair &row = table[blockIdx.z];
    CloudArgs a = row.a;
    const int level = blockIdx.x / row.sk.strips;
    const CloudLevel &lv = row.sk.lv[level];
    a.dx += lv.plane;
    a.dy += lv.plane;
    if (a.conf) a.conf += lv.plane;
    a.left_margin = lv.left_margin;
    a.upper_margin = lv.upper_margin;
    a.scale = lv.scale;
    cloud_tile<true, Form>(a, CloudResize{}, P1q, P2q, &row.sk, level);
}

// The merged cloud of several windows' stacks: the workgroup's entry from its strip; the entry's row of the table in device memory gives its
// planes and mapping into the workgroup's copy of the arguments; its rectangle list is read from the table ONCE, a lane a rectangle, into
// LDS, and reduced from there to the tile's row masks and dense run starts (MultiTile, above cloud_tile).  A tile wholly inside one
// rectangle returns at once (the workgroup that writes the size stays).
template <int Form>
__global__ __launch_bounds__(256) void k_triangulate_fovea(CloudArgs a, Proj P1q, Proj P2q, CloudMulti mu)
{
    static_assert(Form == kTriMultiCount || Form == kTriMulti, "the forms of several windows' stacks");
    __shared__ unsigned long long omask[kCloudTC];
    __shared__ long long run[kCloudTC];
    __shared__ CloudRect rects[kCloudMaxRects];
    const int t = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
    const int strips = (a.wc + kCloudTC - 1) / kCloudTC;
    const int e = tx / strips;
    const CloudEntry &en = mu.table[e];
    const int nrect = min(en.nrect, kCloudMaxRects), nseg = min(en.nseg, kCloudMaxSegs);
    const int c0 = (tx - e * strips) * kCloudTC, r0 = ty * kCloudTR;
    const int c1 = min(c0 + kCloudTC, a.wc), r1 = min(r0 + kCloudTR, a.hc);
    if (t < nrect) rects[t] = en.rect[t];
    __syncthreads();
    bool whole = false;
    for (int i = 0; i < nrect; i++) {
        const CloudRect q = rects[i];
        whole = whole || (c0 >= q.cx0 && c1 <= q.cx1 && r0 >= q.cy0 && r1 <= q.cy1);
    }
    if (whole && !(ty == 0 && tx == (a.compact ? (int)gridDim.x - 1 : 0))) {
        if (Form == kTriMultiCount && t < kCloudTC && c0 + t < a.wc) a.cnt[(size_t)(e * a.wc + c0 + t) * a.nchunk + ty] = 0;
        return;
    }
    if (t < kCloudTC) {
        const int ci = c0 + t;
        unsigned long long m = 0;
        for (int i = 0; i < nrect; i++) {
            const CloudRect q = rects[i];
            if (ci >= q.cx0 && ci < q.cx1) m |= row_bits(q.cy0 - r0, q.cy1 - r0);
        }
        omask[t] = m;
        if (Form == kTriMulti && !a.compact) {
            int above = 0;  // the left-out rows of this column above the tile
            for (int ch = 0; ch < ty; ch++) {
                unsigned long long u = 0;
                for (int i = 0; i < nrect; i++) {
                    const CloudRect q = rects[i];
                    if (ci >= q.cx0 && ci < q.cx1) u |= row_bits(q.cy0 - ch * kCloudTR, q.cy1 - ch * kCloudTR);
                }
                above += __builtin_popcountll(u);
            }
            int sg = 0;     // the column's segment: the last one that starts at or before it
            for (int i = 1; i < nseg; i++)
                if (en.seg_x[i] <= ci) sg = i;
            run[t] = en.first + (long long)en.seg_first[sg] + (long long)(ci - en.seg_x[sg]) * en.seg_rows[sg] + (r0 - above);
        }
    }
    __syncthreads();
    a.dx = en.dx;
    a.dy = en.dy;
    a.conf = a.compact ? en.conf : nullptr;
    a.left_margin = en.left_margin;
    a.upper_margin = en.upper_margin;
    a.scale = en.scale;
    const MultiTile mt{omask, run};
    cloud_tile<true, Form>(a, CloudResize{}, P1q, P2q, nullptr, e, &mu, &mt);
}

int cloud_strips(int wc) { return (wc + kCloudTC - 1) / kCloudTC; }
int cloud_chunks(int hc) { return (hc + kCloudTR - 1) / kCloudTR; }

void launch_point_cloud(hipStream_t st, const CloudArgs &args, bool fovea, const double *P1, const double *P2, const CloudResize *rz)
{
    Proj a, b;
    for (int k = 0; k < 12; k++) { a.m[k] = P1[k]; b.m[k] = P2[k]; }
    using Kern = void (*)(CloudArgs, Proj, Proj, CloudResize);
    const Kern count = rz ? (fovea ? (Kern)k_triangulate_fovea<kTriResizedCount> : (Kern)k_triangulate<kTriResizedCount>)
                          : (fovea ? (Kern)k_triangulate_fovea<kTriCloudCount> : (Kern)k_triangulate<kTriCloudCount>);
    const Kern cloud = rz ? (fovea ? (Kern)k_triangulate_fovea<kTriResized> : (Kern)k_triangulate<kTriResized>)
                          : (fovea ? (Kern)k_triangulate_fovea<kTriCloud> : (Kern)k_triangulate<kTriCloud>);
    const dim3 grid(cloud_strips(args.wc), args.nchunk);
    const CloudResize r = rz ? *rz : CloudResize{};
    if (args.compact) UGSM_LAUNCH(count, grid, dim3(256), 0, st, args, a, b, r);
    UGSM_LAUNCH(cloud, grid, dim3(256), 0, st, args, a, b, r);
}

void launch_point_cloud_stack(hipStream_t st, const CloudArgs &args, const CloudStack &sk, const double *P1, const double *P2)
{
    Proj a, b;
    for (int k = 0; k < 12; k++) { a.m[k] = P1[k]; b.m[k] = P2[k]; }
    const dim3 grid(sk.F * sk.strips, args.nchunk);
    using Kern = void (*)(CloudArgs, Proj, Proj, CloudStack);
    const Kern count = k_triangulate_fovea<kTriStackCount>, cloud = k_triangulate_fovea<kTriStack>;
    if (args.compact) UGSM_LAUNCH(count, grid, dim3(256), 0, st, args, a, b, sk);
    UGSM_LAUNCH(cloud, grid, dim3(256), 0, st, args, a, b, sk);
}

void launch_point_cloud_multi(hipStream_t st, const CloudArgs &args, const CloudMulti &mu, const double *P1, const double *P2)
{
    Proj a, b;
    for (int k = 0; k < 12; k++) { a.m[k] = P1[k]; b.m[k] = P2[k]; }
    const dim3 grid(mu.E * cloud_strips(args.wc), args.nchunk);
    using Kern = void (*)(CloudArgs, Proj, Proj, CloudMulti);
    const Kern count = k_triangulate_fovea<kTriMultiCount>, cloud = k_triangulate_fovea<kTriMulti>;
    if (args.compact) UGSM_LAUNCH(count, grid, dim3(256), 0, st, args, a, b, mu);
    UGSM_LAUNCH(cloud, grid, dim3(256), 0, st, args, a, b, mu);
}

void launch_point_cloud_batch(hipStream_t st, const CloudPair *d_table, int n, const CloudPair &shape, bool stack, const double *P1, const double *P2)
{
    Proj a, b;
    for (int k = 0; k < 12; k++) { a.m[k] = P1[k]; b.m[k] = P2[k]; }
    using Kern = void (*)(const CloudPair *, Proj, Proj);
    const Kern count = stack ? (Kern)k_triangulate_fovea<kTriStackCount> : (Kern)k_triangulate<kTriCloudCount>;
    const Kern cloud = stack ? (Kern)k_triangulate_fovea<kTriStack> : (Kern)k_triangulate<kTriCloud>;
    const dim3 grid(stack ? shape.sk.F * shape.sk.strips : cloud_strips(shape.a.wc), shape.a.nchunk, n);
    if (shape.a.compact) UGSM_LAUNCH(count, grid, dim3(256), 0, st, d_table, a, b);
    UGSM_LAUNCH(cloud, grid, dim3(256), 0, st, d_table, a, b);
}

// =========================================================================================
// one step of hierarchicalDisparity (MatchGPULib.cpp:2643-2683) -- upsample the coarser
// full-frame field by partsubsampleDispKernel (MatchLib.cu:435-462: dst = s * src[tex((x+.5)/s), tex((y+.5)/s)],
// every channel scaled, confidence included) and paste the finer level's fovea at its crop origin, fused: a
// pasted pixel never computes the upsample it would overwrite.  HBM-bound (12 B written per pixel).
// =========================================================================================
__global__ __launch_bounds__(256) void k_upsample_paste(const float *__restrict__ src3, int W, int H, float *__restrict__ dst3, int W2, int H2,
                                                        const float *__restrict__ fovH_, const float *__restrict__ fovV_, const float *__restrict__ fovC_,
                                                        int fovW, int fovH, int org_x, int org_y)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    if (ix >= W2) return;
    const float s = (float)1.41421356;
    const size_t n = (size_t)W * H, n2 = (size_t)W2 * H2, at2 = (size_t)iy * W2 + ix;
    const int fx = ix - org_x, fy = iy - org_y;
    if (fx >= 0 && fx < fovW && fy >= 0 && fy < fovH) {
        const size_t fa = (size_t)fy * fovW + fx;
        dst3[at2] = fovH_[fa];
        dst3[n2 + at2] = fovV_[fa];
        dst3[2 * n2 + at2] = fovC_[fa];
    } else {
        const size_t at = (size_t)tex_index(((float)iy + 0.5f) / s, H) * W + tex_index(((float)ix + 0.5f) / s, W);
        dst3[at2] = s * src3[at];
        dst3[n2 + at2] = s * src3[n + at];
        dst3[2 * n2 + at2] = s * src3[2 * n + at];
    }
}

void launch_upsample_paste(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, const float *fovH_, const float *fovV_,
                           const float *fovC_, int fovW, int fovH, int org_x, int org_y)
{
    UGSM_LAUNCH(k_upsample_paste, dim3((W2 + 255) / 256, H2), dim3(256), 0, st, src3, W, H, dst3, W2, H2, fovH_, fovV_, fovC_, fovW, fovH,
                       org_x, org_y);
}

// The same step over the stacks of pw.n windows of one pair (ugsm_reconstruct_full_multi; PasteWindows, ugsm_launch.hpp): a pixel inside
// window k takes stack k's value -- the HIGHEST such k where windows overlap, found by a loop over the uniform table -- and a pixel inside
// none computes the upsample.  fov0: this level's dx plane in stack 0; its dy and conf planes lie fov_plane, 2 fov_plane floats behind.
// pw.n == 1: the kernel above, operation for operation.
__global__ __launch_bounds__(256) void k_upsample_paste(const float *__restrict__ src3, int W, int H, float *__restrict__ dst3, int W2, int H2,
                                                        const float *__restrict__ fov0, size_t fov_plane, int fovW, int fovH, PasteWindows pw)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    if (ix >= W2) return;
    const float s = (float)1.41421356;
    const size_t n = (size_t)W * H, n2 = (size_t)W2 * H2, at2 = (size_t)iy * W2 + ix;
    int k = -1;
    for (int j = 0; j < pw.n; j++) {
        const int fx = ix - pw.org_x[j], fy = iy - pw.org_y[j];
        if (fx >= 0 && fx < fovW && fy >= 0 && fy < fovH) k = j;
    }
    if (k >= 0) {
        const float *const fov = shifted(fov0, pw.stack[k]);
        const size_t fa = (size_t)(iy - pw.org_y[k]) * fovW + (ix - pw.org_x[k]);
        dst3[at2] = fov[fa];
        dst3[n2 + at2] = fov[fov_plane + fa];
        dst3[2 * n2 + at2] = fov[2 * fov_plane + fa];
    } else {
        const size_t at = (size_t)tex_index(((float)iy + 0.5f) / s, H) * W + tex_index(((float)ix + 0.5f) / s, W);
        dst3[at2] = s * src3[at];
        dst3[n2 + at2] = s * src3[n + at];
        dst3[2 * n2 + at2] = s * src3[2 * n + at];
    }
}

void launch_upsample_paste_multi(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, const float *fov0, size_t fov_plane,
                                 int fovW, int fovH, const PasteWindows &pw)
{
    UGSM_LAUNCH(k_upsample_paste, dim3((W2 + 255) / 256, H2), dim3(256), 0, st, src3, W, H, dst3, W2, H2, fov0, fov_plane, fovW, fovH, pw);
}

// The pointwise form (k_restrict_stack in the statistics; ugsm_submit_foveated_warm -- no reference counterpart, DESIGN.md section 8;
// RestrictStack, ugsm_launch.hpp): one thread per pixel of the fw x fh starting field of fovea level k of entry e, blockIdx.z = e x (F - s) +
// (k - s), all three planes -- they share the descent.  Window pixel (ix, iy) is level-k pixel (ix + nox[k], iy + noy[k]); its level-0 site is
// restrict_site's; from there the rule of the kernels above is walked from level 0 upwards: level l < F-1 holds the value where the site
// lies inside the prior's window of that level, otherwise it is s * (level l + 1 at tex_index((c + .5f) / s)), the very expressions above.
// The walk's level is uniform (the windows' origins and the levels' sizes come from scalar loads); a lane that has found its level stops
// moving, and the wave leaves the loop when every lane has.  The multiplications by s follow, one per level descended, each rounded on its
// own; then the restriction's value transform (k_seed's restriction form).  Nothing is read outside the prior: a window test precedes every
// read of a level below F-1, and tex_index clamps to level F-1's own size.
template <bool kTable>
__global__ __launch_bounds__(256) void k_upsample_paste(const float *__restrict__ prior0, float *__restrict__ stack0, float *__restrict__ work0, RestrictStack rs)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    const int nl = rs.F - rs.s;
    const int e = blockIdx.z / nl, k = rs.s + (int)blockIdx.z - e * nl;
    const RestrictStackRow &row = kTable ? rs.table[e] : rs.rows[e];
    if (ix >= rs.fw) return;
    const float s = (float)1.41421356;
    const int half = k >> 1, odd = k & 1;
    int x = restrict_site(ix + row.nox[k], half, odd, rs.W);
    int y = restrict_site(iy + row.noy[k], half, odd, rs.H);
    const float *const src = shifted(prior0, row.prior);
    const size_t fn = (size_t)rs.fw * rs.fh;
    size_t at, plane;
    int depth = 0;
    if (rs.field) {
        at = (size_t)y * rs.W + x;
        plane = (size_t)rs.W * rs.H;
    } else {
        plane = (size_t)rs.F * fn;
        bool found = false;
        at = 0;
        for (int l = 0; l < rs.F - 1; l++) {
            const int fx = x - row.pox[l], fy = y - row.poy[l];
            if (!found && fx >= 0 && fx < rs.fw && fy >= 0 && fy < rs.fh) {
                found = true;
                depth = l;
                at = (size_t)l * fn + (size_t)fy * rs.fw + fx;
            }
            if (!found) {
                x = tex_index(((float)x + 0.5f) / s, rs.w[l + 1]);
                y = tex_index(((float)y + 0.5f) / s, rs.h[l + 1]);
            }
            if (__ballot(!found) == 0) break;
        }
        if (!found) {
            depth = rs.F - 1;
            at = (size_t)(rs.F - 1) * fn + (size_t)y * rs.fw + x;
        }
    }
    float v0 = src[at], v1 = src[plane + at], v2 = src[2 * plane + at];
    for (int j = 0; j < depth; j++) {
        v0 = s * v0;
        v1 = s * v1;
        v2 = s * v2;
    }
    if (odd) {
        v0 = (float)((double)v0 / UGSM_SCALE);
        v1 = (float)((double)v1 / UGSM_SCALE);
    }
    if (half) {
        const float scale = __int_as_float((127 - half) << 23);  // 2^-half
        v0 = v0 * scale;
        v1 = v1 * scale;
    }
    const size_t o = (size_t)iy * rs.fw + ix;
    if (work0 && k == rs.s) {
        float *const dst = shifted(work0, row.work);
        dst[o] = v0;
        dst[fn + o] = v1;
        dst[2 * fn + o] = v2;
    } else {
        float *const dst = shifted(stack0, row.dst) + (size_t)k * fn;
        const size_t stack_plane = (size_t)rs.F * fn;
        dst[o] = v0;
        dst[stack_plane + o] = v1;
        dst[2 * stack_plane + o] = v2;
    }
}

bool launch_restrict_stack(hipStream_t st, const float *prior0, float *stack0, float *work0, RestrictStack rs, const RestrictStackRow *rows)
{
    if (!rows || rs.n < 1 || rs.n > kMaxBatch || rs.F < 2 || rs.F > kCloudMaxLevels || rs.s < 0 || rs.s >= rs.F) return false;
    if (rs.fw < 1 || rs.fh < 1 || rs.w[rs.F - 1] != rs.fw || rs.h[rs.F - 1] != rs.fh || rs.w[0] != rs.W || rs.h[0] != rs.H) return false;
    if (!rs.table && rs.n > kRestrictStackByValue) return false;
    for (int e = 0; e < rs.n; e++) {
        const RestrictStackRow &r = rows[e];
        for (int k = rs.s; k < rs.F; k++)
            if (r.nox[k] < 0 || r.noy[k] < 0 || r.nox[k] + rs.fw > rs.w[k] || r.noy[k] + rs.fh > rs.h[k]) return false;
        for (int l = 0; !rs.field && l < rs.F - 1; l++)
            if (r.pox[l] < 0 || r.poy[l] < 0 || r.pox[l] + rs.fw > rs.w[l] || r.poy[l] + rs.fh > rs.h[l]) return false;
        if (!rs.table) rs.rows[e] = r;
    }
    const dim3 grid((rs.fw + 255) / 256, rs.fh, rs.n * (rs.F - rs.s));
    if (rs.table) UGSM_LAUNCH(k_upsample_paste<true>, grid, dim3(256), 0, st, prior0, stack0, work0, rs);
    else UGSM_LAUNCH(k_upsample_paste<false>, grid, dim3(256), 0, st, prior0, stack0, work0, rs);
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
    void (*const rows)(const float *, const float *, int, int, double *) = k_wdiff_rows;  // (the field forms, among the residual's below)
    void (*const total)(const double *, int, double *) = k_wdiff_total;
    UGSM_LAUNCH(rows, dim3(H), dim3(64), 0, st, newd3, oldd3, W, H, rowsum);
    UGSM_LAUNCH(total, dim3(1), dim3(64), 0, st, (const double *)rowsum, H, out3);
}

// The photometric residual of a match (ugsm_photometric_residual[_fovea]; ResidualArgs, ugsm_launch.hpp): row f-4's rule on a left plane
// and the warped right plane, the warp never stored.  Per pixel and channel t = fabsf(L_c - R_c[warp]) in float, t = t * conf in float
// (conf null: 1.0f); S_c = sum(t), C = sum(conf) in the order above: a wave per row, lane l its columns x = l (mod 64) left to right, then the
// 64 lane sums in lane order.  kResidualRows rows per workgroup, blockIdx.y the level of a stack; a pixel's left and right values are read
// once for the three channels.  The total form: one wave per level adds the rows the same way.  No atomics: the same bytes every run.
constexpr int kResidualRows = 4;
template <int L>
__global__ __launch_bounds__(64 * kResidualRows) void k_wdiff_rows(ResidualArgs a)
{
    __shared__ double sp[kResidualRows][4][64];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int y = blockIdx.x * kResidualRows + w, level = blockIdx.y;
    const size_t n = (size_t)a.W * a.H;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    if (y < a.H) {
        const size_t row = (size_t)level * n + (size_t)y * a.W;
#pragma unroll 4
        for (int x = l; x < a.W; x += 64) {
            const float c = a.conf ? a.conf[row + x] : 1.0f;
            const int sx = tex_index(((float)x + 0.5f) + a.dx[row + x], a.W);
            const int sy = tex_index(((float)y + 0.5f) + a.dy[row + x], a.H);
            float lf[3], rf[3];
            if constexpr (L == kInPlanes) {
                const float *const lp = static_cast<const float *>(a.L) + (size_t)level * 3 * n + (size_t)y * a.W + x;
                const float *const rp = static_cast<const float *>(a.R) + (size_t)level * 3 * n + (size_t)sy * a.W + sx;
                for (int k = 0; k < 3; k++) {
                    lf[k] = lp[k * n];
                    rf[k] = rp[k * n];
                }
            } else {
                InPix<L>::loadf(static_cast<const uint8_t *>(a.L) + (size_t)y * a.stride + InPix<L>::bpp * x, lf);
                InPix<L>::loadf(static_cast<const uint8_t *>(a.R) + (size_t)sy * a.stride + InPix<L>::bpp * sx, rf);
                if (InPix<L>::mono) {
                    lf[1] = lf[2] = lf[0];
                    rf[1] = rf[2] = rf[0];
                }
            }
            for (int k = 0; k < 3; k++) {
                float t = fabsf(lf[k] - rf[k]);
                t = t * c;
                p[k] += (double)t;
            }
            p[3] += (double)c;
        }
    }
    for (int k = 0; k < 4; k++) sp[w][k][l] = p[k];
    __syncthreads();
    if (l < 4 && y < a.H) {
        double r = 0.0;
        for (int i = 0; i < 64; i++) r += sp[w][l][i];
        a.rowsum[((size_t)level * a.H + y) * 4 + l] = r;
    }
}
__global__ __launch_bounds__(64) void k_wdiff_total(ResidualArgs a, double *__restrict__ sums)
{
    __shared__ double sp[4][64];
    const int l = threadIdx.x, level = blockIdx.x;
    const double *const rowsum = a.rowsum + (size_t)level * a.H * 4;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8  // (a lane's rows are independent loads: eight rows in flight, added in the order they come in)
    for (int y = l; y < a.H; y += 64)
        for (int k = 0; k < 4; k++) p[k] += rowsum[(size_t)y * 4 + k];
    for (int k = 0; k < 4; k++) sp[k][l] = p[k];
    __syncthreads();
    if (l < 4) {
        double r = 0.0;
        for (int i = 0; i < 64; i++) r += sp[l][i];
        sums[level * 4 + l] = r;
    }
}
void launch_residual(hipStream_t st, const ResidualArgs &a, int in, double *sums)
{
    using Rows = void (*)(ResidualArgs);
    using Total = void (*)(ResidualArgs, double *);
    const dim3 grid((a.H + kResidualRows - 1) / kResidualRows, a.levels);
    if (in == kInPlanes) {
        const Rows rows = k_wdiff_rows<kInPlanes>;
        UGSM_LAUNCH(rows, grid, dim3(64 * kResidualRows), 0, st, a);
    } else {
        const bool words = input_words_aligned(static_cast<const uint8_t *>(a.L), a.stride, nullptr) &&
                           input_words_aligned(static_cast<const uint8_t *>(a.R), a.stride, nullptr);
        with_layout(input_layout(in, words), [&](auto layout) {
            const Rows rows = k_wdiff_rows<decltype(layout)::value>;
            UGSM_LAUNCH(rows, grid, dim3(64 * kResidualRows), 0, st, a);
        });
    }
    const Total total = k_wdiff_total;
    UGSM_LAUNCH(total, dim3(a.levels), dim3(64), 0, st, a, sums);
}

}  // namespace ugsm
