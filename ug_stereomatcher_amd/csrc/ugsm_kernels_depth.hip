// ugsm_kernels_depth.hip -- SURVEY 8f row f-1: triangulation of a match into X, Y, Z planes and into REP 118 depth images.
//
// k_triangulate / k_triangulate_fovea: the X, Y, Z planes and, as their depth forms, the REP 118 depth image -- k_triangulate's frame forms: the
// depth image of the whole frame from a fovea stack.  A pixel's point is ugsm_tri.hpp's, which the cloud kernels (ugsm_kernels_cloud.hip)
// share.  HBM-bound.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#include "ugsm_tri.hpp"

namespace ugsm {

// =========================================================================================
// The depth image (ugsm_depth_image[_fovea]): the reference's range_map / res_range_map (getPointCloud.cpp:730-758, :813-841, :951-1021) as a
// REP 118 image, row-major.  Z is tri_of's (the planes' Z, bit for bit) or resized_point's (the resized clouds' z, bit for bit); then, every
// operation in binary32 and rounded on its own:
//   valid  Z finite, z_min <= Z <= z_max, and conf >= min_conf where there is a confidence plane (a NaN confidence fails);
//   32F    m = Z * unit where valid, else the quiet NaN 0x7FC00000;
//   16U    u = (m * 1000.0f) + 0.5f, valid only with 1.0f <= u < 65536.0f; (uint16_t)u where valid, else 0.
// The valid pixels are counted with one ballot and popcount per pixel of a thread's run, summed over the runs a wave walks and then over the
// workgroup's four waves through LDS, and added with ONE 64-bit integer atomic per workgroup: a sum of integers, the same from run to run.
// (One atomic per wave of a grid of one run per thread -- 33 k to 66 k adds to one word at 16 MP -- made the launch five to eleven times
// longer than the same launch without the count: DESIGN.md section 8.  Hence the capped grid, kDepthMaxBlocks, and the workgroup's sum.)
// =========================================================================================
template <bool U16>
__device__ __forceinline__ bool depth_element(const DepthArgs &d, float Z, float conf, unsigned &bits)
{
    bool valid = __builtin_isfinite(Z) && Z >= d.z_min && Z <= d.z_max;
    if (d.conf) valid = valid && conf >= d.min_conf;
    const float m = Z * d.unit;
    if (U16) {
        const float u = (m * 1000.0f) + 0.5f;
        valid = valid && u >= 1.0f && u < 65536.0f;
        bits = valid ? (unsigned)u : 0u;
    } else {
        bits = valid ? __float_as_uint(m) : 0x7FC00000u;
    }
    return valid;
}

constexpr int kDepthMaxBlocks = 2048;  // workgroups of a depth launch per level: about what the chip holds at once; a workgroup walks the rest

// count: the wave's valid pixels (the same in every lane)
__device__ __forceinline__ void depth_count(const DepthArgs &d, int level, unsigned count)
{
    __shared__ unsigned waves[4];
    if (!d.valid) return;  // (uniform)
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = count;
    __syncthreads();
    const unsigned total = waves[0] + waves[1] + waves[2] + waves[3];
    if (threadIdx.x == 0 && total) atomicAdd(d.valid + level, (unsigned long long)total);
}

// The plain form: 8 to 12 bytes in, 2 or 4 out per pixel; only Z is live, so tri_point's X and Y numerators fall away.  The
// level's pw * ph pixels are indexed flat -- planes and image are contiguous -- and a thread owns a run of 16 bytes of the image: 8 pixels of
// 16U, 4 of 32F.  Run r holds the pixels [head - Run + r Run, head + r Run), head = the pixels in front of the image's first 16-byte boundary
// (0 .. Run-1): run 0 is the head, the last run the tail, and both go element by element; every run between them is stored with one 16-byte
// store, and loaded with 16-byte loads where dx, dy and conf are 16-byte aligned at pixel `head` too (else with 4-byte loads).  Nothing but a
// pixel's own bytes is written.  A workgroup takes 256 runs at a time and walks on by the grid's width.
template <bool Fovea, bool U16, bool L, class Src = PlaneSrc>
__device__ __forceinline__ void depth_run(const CloudArgs &a, const DepthArgs &d, const Proj &P1q, const Proj &P2q, int level, const Lens *ln,
                                          const Src *src = nullptr)
{
    constexpr int Size = U16 ? 2 : 4, Run = 16 / Size;
    const int n = a.pw * a.ph;
    char *const out = reinterpret_cast<char *>(d.out) + (size_t)level * n * Size;
    const int head = (int)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) / Size;
    const bool wide = ((reinterpret_cast<uintptr_t>(a.dx + head) | reinterpret_cast<uintptr_t>(a.dy + head) |
                        (a.conf ? reinterpret_cast<uintptr_t>(a.conf + head) : (uintptr_t)0)) & 15) == 0;
    const int runs = (n - head + Run - 1) / Run + 1;  // run 0 (the head) .. the tail's
    unsigned count = 0;
    for (int r0 = blockIdx.x * 256; r0 < runs; r0 += gridDim.x * 256) {  // (uniform over the workgroup)
        const int i0 = head - Run + (r0 + (int)threadIdx.x) * Run;
        const bool full = i0 >= 0 && i0 + Run <= n;
        float ddx[Run], ddy[Run], cf[Run];
        if constexpr (!Src::kPlanes) {  // the run's pixels side by side through the source (a pixel outside the image: pixel (0, 0)'s, unused)
            int px[Run], py[Run];
            const int first = max(i0, 0);
            int fy = first / a.pw, fx = first - fy * a.pw;
#pragma unroll
            for (int e = 0; e < Run; e++) {
                const int i = i0 + e;
                const bool in = i >= 0 && i < n;
                px[e] = in ? fx : 0;
                py[e] = in ? fy : 0;
                if (in && ++fx == a.pw) {
                    fx = 0;
                    fy++;
                }
            }
            src->template fetch<Run>(px, py, ddx, ddy, cf);
        } else if (full && wide) {
#pragma unroll
            for (int q = 0; q < Run / 4; q++) {
                const float4 vx = reinterpret_cast<const float4 *>(a.dx + i0)[q], vy = reinterpret_cast<const float4 *>(a.dy + i0)[q];
                const float4 vc = a.conf ? reinterpret_cast<const float4 *>(a.conf + i0)[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                ddx[4 * q] = vx.x, ddx[4 * q + 1] = vx.y, ddx[4 * q + 2] = vx.z, ddx[4 * q + 3] = vx.w;
                ddy[4 * q] = vy.x, ddy[4 * q + 1] = vy.y, ddy[4 * q + 2] = vy.z, ddy[4 * q + 3] = vy.w;
                cf[4 * q] = vc.x, cf[4 * q + 1] = vc.y, cf[4 * q + 2] = vc.z, cf[4 * q + 3] = vc.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < Run; e++) {
                const int i = i0 + e;
                const bool in = i >= 0 && i < n;
                ddx[e] = in ? a.dx[i] : 0.0f;
                ddy[e] = in ? a.dy[i] : 0.0f;
                cf[e] = in && a.conf ? a.conf[i] : 0.0f;
            }
        }
        const int first = max(i0, 0);  // the run's first pixel inside the image: (xx, yy) walks on from there
        int yy = first / a.pw, xx = first - yy * a.pw;
        unsigned bits[Run];
#pragma unroll
        for (int e = 0; e < Run; e++) {
            const int i = i0 + e;
            bool valid = false;
            bits[e] = 0;
            if (full || (i >= 0 && i < n)) {
                float x1, y1, X, Y, Z;
                tri_of<Fovea, L>(a, P1q, P2q, xx, yy, ddx[e], ddy[e], x1, y1, X, Y, Z, ln);
                valid = depth_element<U16>(d, Z, cf[e], bits[e]);
                if (++xx == a.pw) {
                    xx = 0;
                    yy++;
                }
            }
            count += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
        }
        if (full) {
            uint4 v;
            if constexpr (U16) v = make_uint4(bits[0] | bits[1] << 16, bits[2] | bits[3] << 16, bits[4] | bits[5] << 16, bits[6] | bits[7] << 16);
            else v = make_uint4(bits[0], bits[1], bits[2], bits[3]);
            *reinterpret_cast<uint4 *>(out + (size_t)i0 * Size) = v;
        } else {
#pragma unroll
            for (int e = 0; e < Run; e++) {
                const int i = i0 + e;
                if (i < 0 || i >= n) continue;
                if (U16) reinterpret_cast<unsigned short *>(out)[i] = (unsigned short)bits[e];
                else reinterpret_cast<unsigned *>(out)[i] = bits[e];
            }
        }
    }
    depth_count(d, level, count);
}

// The resized form: pixel (ii, jj) of the dw x dh map, a thread a pixel (the image is factor^2 of the planes, and a pixel costs sixteen
// tri_at).  Z is the z of resized_point's record -- the resized clouds' own routine, with no colour to read and nothing to keep (`a` is a
// dense cloud's: compact 0) --; the confidence is read where that routine registers the pixel, (xx, yy) = ((int)((float)ii / factor),
// (int)((float)jj / factor)), inside the plane as there.
template <bool Fovea, bool U16, bool L, class Src = PlaneSrc>
__device__ __forceinline__ void depth_resized(const CloudArgs &a, const DepthArgs &d, const Proj &P1q, const Proj &P2q, int level, const Lens *ln,
                                              const Src *src = nullptr)
{
    const int n = d.dw * d.dh;
    unsigned count = 0;
    for (int i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {  // (uniform over the workgroup)
        const int i = i0 + (int)threadIdx.x;
        bool valid = false;
        if (i < n) {
            const int jj = i / d.dw, ii = i - jj * d.dw;
            const int xx = min((int)((float)ii / d.rz.factor), a.pw - 1), yy = min((int)((float)jj / d.rz.factor), a.ph - 1);
            float cf;
            if constexpr (!Src::kPlanes) {
                float ux, uy;
                src->fetch1(xx, yy, ux, uy, cf);
            } else {
                cf = a.conf ? a.conf[(size_t)yy * a.pw + xx] : 0.0f;
            }
            float4 rec;
            resized_point<Fovea, false, true, L, Src>(a, d.rz, P1q, P2q, ii, jj, rec, ln, src);
            unsigned bits;
            valid = depth_element<U16>(d, rec.z, cf, bits);
            const size_t o = (size_t)level * n + i;
            if (U16) reinterpret_cast<unsigned short *>(d.out)[o] = (unsigned short)bits;
            else reinterpret_cast<unsigned *>(d.out)[o] = bits;
        }
        count += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
    }
    depth_count(d, level, count);
}

// What k_triangulate / k_triangulate_fovea emit (template parameter): the X, Y, Z planes, or the depth image in its four forms.  The planes'
// instances keep the argument list and the body they had as plain kernels; a depth instance takes its DepthArgs where they take the planes.
// k_triangulate alone has the frame forms: the depth image of the WHOLE frame from a fovea stack (ugsm_depth_image_fovea_full / _multi;
// DepthFrame, ugsm_launch.hpp) -- the four depth forms over the W x H frame, the same runs, stores, grid and count, every (dx, dy, conf) a
// FrameSrc descent instead of a plane read; dispx / dispy are then stack 0's dx and dy planes.  kEmitFrame + a depth form: the window in the
// arguments; kEmitFrameTable + a depth form: the n > 1 windows read from the table.
enum TriEmit : int { kEmitPlanes = 0, kEmitDepth32F = 1, kEmitDepth16U = 2, kEmitResized32F = 3, kEmitResized16U = 4, kEmitFrame = 4, kEmitFrameTable = 8 };
constexpr bool emit_frame(int emit) { return emit > kEmitFrame; }
constexpr bool emit_table(int emit) { return emit > kEmitFrameTable; }
constexpr int emit_depth(int emit) { return emit > kEmitFrameTable ? emit - kEmitFrameTable : emit > kEmitFrame ? emit - kEmitFrame : emit; }
struct DepthFrameArgs {
    DepthArgs d;
    DepthFrame fr;
};
template <int Emit>
struct TriOut {
    using field = std::conditional_t<emit_frame(Emit), DepthFrameArgs, DepthArgs>;
    using fovea = DepthFoveaArgs;
};
template <>
struct TriOut<kEmitPlanes> {
    using field = float *__restrict__;
    using fovea = float *__restrict__;
};

template <int Emit, class... LensArg>
__global__ __launch_bounds__(256) void k_triangulate(const float *__restrict__ dispx, const float *__restrict__ dispy, int W, int H, Proj P1q, Proj P2q,
                                                     typename TriOut<Emit>::field out, LensArg... lens)
{
    constexpr bool L = sizeof...(LensArg) != 0;
    [[maybe_unused]] const Lens *const ln = lens_of(lens...);
    if constexpr (Emit == kEmitPlanes) {
        float *__restrict__ xyz = out;
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
        if constexpr (L) tri_point_lens(*ln, x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
        else tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
        xyz[at] = X;
        xyz[n + at] = Y;
        xyz[2 * n + at] = Z;
    } else if constexpr (emit_frame(Emit)) {
        constexpr int Form = emit_depth(Emit);
        CloudArgs a{};
        a.conf = out.d.conf;
        a.pw = W;
        a.ph = H;
        const FrameSrc<emit_table(Emit)> src{dispx, dispy, out.d.conf, &out.fr};
        if constexpr (Form == kEmitDepth32F || Form == kEmitDepth16U) depth_run<false, Form == kEmitDepth16U, L>(a, out.d, P1q, P2q, 0, ln, &src);
        else depth_resized<false, Form == kEmitResized16U, L>(a, out.d, P1q, P2q, 0, ln, &src);
    } else {
        CloudArgs a{};
        a.dx = dispx;
        a.dy = dispy;
        a.conf = out.conf;
        a.pw = W;
        a.ph = H;
        if constexpr (Emit == kEmitDepth32F || Emit == kEmitDepth16U) depth_run<false, Emit == kEmitDepth16U, L>(a, out, P1q, P2q, 0, ln);
        else depth_resized<false, Emit == kEmitResized16U, L>(a, out, P1q, P2q, 0, ln);
    }
}

// get3DPoint, foveated branch (getPointCloud.cpp:892-903): level src_level of the (F*fovH) x fovW stacks, pixel
// coordinates mapped into the full-resolution frame by mapXcoord / mapYcoord (:387-421).  Those take an int, so the
// right-image coordinate xx + disparity is truncated toward zero before scaling -- kept as in the reference.
// The depth forms: blockIdx.y = the level among the launch's (src_level the first), its mapping from the table.
template <int Emit, class... LensArg>
__global__ __launch_bounds__(256) void k_triangulate_fovea(const float *__restrict__ stackx, const float *__restrict__ stacky, int fovW, int fovH,
                                                           int src_level, int left_margin, int upper_margin, float scale, Proj P1q, Proj P2q,
                                                           typename TriOut<Emit>::fovea out, LensArg... lens)
{
    constexpr bool L = sizeof...(LensArg) != 0;
    [[maybe_unused]] const Lens *const ln = lens_of(lens...);
    if constexpr (Emit == kEmitPlanes) {
        float *__restrict__ xyz = out;
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
        if constexpr (L) tri_point_lens(*ln, x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
        else tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
        xyz[at] = X;
        xyz[n + at] = Y;
        xyz[2 * n + at] = Z;
    } else {
        const int k = blockIdx.y, level = src_level + k;
        const size_t plane = (size_t)level * fovW * fovH;
        CloudArgs a{};
        a.dx = stackx + plane;
        a.dy = stacky + plane;
        a.conf = out.d.conf ? out.d.conf + plane : nullptr;
        a.pw = fovW;
        a.ph = fovH;
        a.left_margin = out.lv.left[level];
        a.upper_margin = out.lv.upper[level];
        a.scale = out.lv.scale[level];
        if constexpr (Emit == kEmitDepth32F || Emit == kEmitDepth16U) depth_run<true, Emit == kEmitDepth16U, L>(a, out.d, P1q, P2q, k, ln);
        else depth_resized<true, Emit == kEmitResized16U, L>(a, out.d, P1q, P2q, k, ln);
    }
}

void launch_triangulate(hipStream_t st, const float *dispx, const float *dispy, int W, int H, const double *P1, const double *P2, float *xyz,
                        const Lens *lens)
{
    const Proj a = proj(P1), b = proj(P2);
    UGSM_LAUNCH_LENS(lens, (k_triangulate<kEmitPlanes>), (k_triangulate<kEmitPlanes, Lens>), dim3((W + 255) / 256, H), st, dispx, dispy, W, H, a, b, xyz);
}

void launch_triangulate_fovea(hipStream_t st, const float *stackx, const float *stacky, int fovW, int fovH, int src_level, int left_margin,
                              int upper_margin, float scale, const double *P1, const double *P2, float *xyz, const Lens *lens)
{
    const Proj a = proj(P1), b = proj(P2);
    UGSM_LAUNCH_LENS(lens, (k_triangulate_fovea<kEmitPlanes>), (k_triangulate_fovea<kEmitPlanes, Lens>), dim3((fovW + 255) / 256, fovH), st, stackx, stacky,
                     fovW, fovH, src_level, left_margin, upper_margin, scale, a, b, xyz);
}

// workgroups of a depth launch over one level of n pixels: the plain forms' runs (n / Run whole ones, the head's and the tail's), the
// resized forms' pixels
static unsigned depth_blocks(long long n, bool resized, bool u16)
{
    const long long threads = resized ? n : n / (u16 ? 8 : 4) + 2;
    const long long blocks = (threads + 255) / 256;
    return (unsigned)(blocks < kDepthMaxBlocks ? blocks : kDepthMaxBlocks);
}

void launch_depth_image(hipStream_t st, const float *dispx, const float *dispy, int W, int H, const double *P1, const double *P2, const DepthArgs &d,
                        bool u16, const Lens *lens)
{
    const Proj a = proj(P1), b = proj(P2);
    using Kern = void (*)(const float *, const float *, int, int, Proj, Proj, DepthArgs);
    using KernLens = void (*)(const float *, const float *, int, int, Proj, Proj, DepthArgs, Lens);
    const bool resized = d.rz.factor < 1.0f;
    const Kern kern = resized ? (u16 ? (Kern)k_triangulate<kEmitResized16U> : (Kern)k_triangulate<kEmitResized32F>)
                              : (u16 ? (Kern)k_triangulate<kEmitDepth16U> : (Kern)k_triangulate<kEmitDepth32F>);
    const KernLens kern_lens = resized ? (u16 ? (KernLens)k_triangulate<kEmitResized16U, Lens> : (KernLens)k_triangulate<kEmitResized32F, Lens>)
                                       : (u16 ? (KernLens)k_triangulate<kEmitDepth16U, Lens> : (KernLens)k_triangulate<kEmitDepth32F, Lens>);
    UGSM_LAUNCH_LENS(lens, kern, kern_lens, dim3(depth_blocks((long long)d.dw * d.dh, resized, u16)), st, dispx, dispy, W, H, a, b, d);
}

void launch_depth_image_fovea(hipStream_t st, const float *stackx, const float *stacky, int fovW, int fovH, int src_level, const double *P1,
                              const double *P2, const DepthFoveaArgs &d, bool u16, const Lens *lens)
{
    const Proj a = proj(P1), b = proj(P2);
    using Kern = void (*)(const float *, const float *, int, int, int, int, int, float, Proj, Proj, DepthFoveaArgs);
    using KernLens = void (*)(const float *, const float *, int, int, int, int, int, float, Proj, Proj, DepthFoveaArgs, Lens);
    const bool resized = d.d.rz.factor < 1.0f;
    const Kern kern = resized ? (u16 ? (Kern)k_triangulate_fovea<kEmitResized16U> : (Kern)k_triangulate_fovea<kEmitResized32F>)
                              : (u16 ? (Kern)k_triangulate_fovea<kEmitDepth16U> : (Kern)k_triangulate_fovea<kEmitDepth32F>);
    const KernLens kern_lens = resized ? (u16 ? (KernLens)k_triangulate_fovea<kEmitResized16U, Lens> : (KernLens)k_triangulate_fovea<kEmitResized32F, Lens>)
                                       : (u16 ? (KernLens)k_triangulate_fovea<kEmitDepth16U, Lens> : (KernLens)k_triangulate_fovea<kEmitDepth32F, Lens>);
    UGSM_LAUNCH_LENS(lens, kern, kern_lens, dim3(depth_blocks((long long)d.d.dw * d.d.dh, resized, u16), d.lv.levels), st, stackx, stacky, fovW, fovH,
                     src_level, 0, 0, 0.0f, a, b, d);
}

template <int Base>
static void launch_depth_frame(hipStream_t st, const float *stackx, const float *stacky, const Proj &a, const Proj &b, const DepthFrameArgs &d, bool u16,
                               const Lens *lens)
{
    using Kern = void (*)(const float *, const float *, int, int, Proj, Proj, DepthFrameArgs);
    using KernLens = void (*)(const float *, const float *, int, int, Proj, Proj, DepthFrameArgs, Lens);
    const bool resized = d.d.rz.factor < 1.0f;
    const Kern kern = resized ? (u16 ? (Kern)k_triangulate<Base + kEmitResized16U> : (Kern)k_triangulate<Base + kEmitResized32F>)
                              : (u16 ? (Kern)k_triangulate<Base + kEmitDepth16U> : (Kern)k_triangulate<Base + kEmitDepth32F>);
    const KernLens kern_lens = resized ? (u16 ? (KernLens)k_triangulate<Base + kEmitResized16U, Lens> : (KernLens)k_triangulate<Base + kEmitResized32F, Lens>)
                                       : (u16 ? (KernLens)k_triangulate<Base + kEmitDepth16U, Lens> : (KernLens)k_triangulate<Base + kEmitDepth32F, Lens>);
    UGSM_LAUNCH_LENS(lens, kern, kern_lens, dim3(depth_blocks((long long)d.d.dw * d.d.dh, resized, u16)), st, stackx, stacky, d.fr.w[0], d.fr.h[0], a, b, d);
}

bool launch_depth_image_frame(hipStream_t st, const float *stackx, const float *stacky, const double *P1, const double *P2, const DepthArgs &d,
                              DepthFrame fr, const FrameWindow *win, bool u16, const Lens *lens)
{
    if (!win || fr.n < 1 || fr.n > kMaxBatch || fr.F < 2 || fr.F > kCloudMaxLevels || (fr.n > 1) != (fr.table != nullptr)) return false;
    if (fr.fw < 1 || fr.fh < 1 || fr.w[fr.F - 1] != fr.fw || fr.h[fr.F - 1] != fr.fh || (long long)fr.F * fr.fw * fr.fh > 0x7fffffffll) return false;
    if ((long long)fr.w[0] * fr.h[0] > (1ll << 28) || d.dw < 1 || d.dh < 1 || d.dw > fr.w[0] || d.dh > fr.h[0]) return false;
    if (!(d.rz.factor < 1.0f) && (d.dw != fr.w[0] || d.dh != fr.h[0])) return false;
    for (int l = 0; l < fr.F; l++)
        if (fr.w[l] < 1 || fr.h[l] < 1) return false;  // (tex_index clamps to n - 1: every read lies inside its level)
    for (int j = 0; j < fr.n; j++)
        for (int l = 0; l < fr.F - 1; l++)
            if (win[j].ox[l] < 0 || win[j].oy[l] < 0 || win[j].ox[l] + fr.fw > fr.w[l] || win[j].oy[l] + fr.fh > fr.h[l]) return false;
    const Proj a = proj(P1), b = proj(P2);
    if (!fr.table) fr.win = win[0];
    const DepthFrameArgs args{d, fr};
    if (fr.table) launch_depth_frame<kEmitFrameTable>(st, stackx, stacky, a, b, args, u16, lens);
    else launch_depth_frame<kEmitFrame>(st, stackx, stacky, a, b, args, u16, lens);
    return true;
}

}  // namespace ugsm
