// ugsm_kernels_warp.hip -- the right image warped by a match, and the photometric residual of a match: the device side of ugsm_warp.cpp.
//
// k_warp_right (MatchGPULib::warpRightImage), k_residual_rows / k_residual_total (row f-4's rule on a left plane and the warped right plane,
// the warp never stored).  HBM-bound.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#include "ugsm_device.hpp"
#include "ugsm_launch.hpp"

namespace ugsm {

// The warp (ugsm_warp_planes, ugsm_warp_right, ugsm_warp_right_fovea): MatchGPULib::warpRightImage, MatchGPULib.cpp:1445-1518 over kernel
// warpAbyB (MatchLib.cu:499-549) -- dst[iy][ix] = src[tex(iy + .5f + dy)][tex(ix + .5f + dx)], K-cost's own fetch (ugsm_kernels_march.hip),
// the value stored as it was fetched.  One template over the source (WarpArgs, ugsm_launch.hpp): kInPlanes -- float planes in, blockIdx.z the
// plane, warped by field z / per_field (one field for every plane, or a fovea stack's level = z / 3); an InLayout -- the 8-bit image in, the
// gathered pixel read once for its three planes.  HBM-bound: 8 B of (dx, dy), one gathered value, 4 (12) B written per thread.
template <int L>
__global__ __launch_bounds__(256) void k_warp_right(WarpArgs a)
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
        const Kern kern = k_warp_right<kInPlanes>;
        UGSM_LAUNCH(kern, grid2(a.W, a.H, a.planes), dim3(256), 0, st, a);
        return;
    }
    const bool words = input_words_aligned(static_cast<const uint8_t *>(a.src), a.stride, nullptr);
    with_layout(input_layout(in, words), [&](auto layout) {
        const Kern kern = k_warp_right<decltype(layout)::value>;
        UGSM_LAUNCH(kern, grid2(a.W, a.H), dim3(256), 0, st, a);
    });
}

// The photometric residual of a match (ugsm_photometric_residual[_fovea]; ResidualArgs, ugsm_launch.hpp): row f-4's rule on a left plane
// and the warped right plane, the warp never stored.  Per pixel and channel t = fabsf(L_c - R_c[warp]) in float, t = t * conf in float
// (conf null: 1.0f); S_c = sum(t), C = sum(conf) in k_wdiff_rows' order: a wave per row, lane l its columns x = l (mod 64) left to right, then the
// 64 lane sums in lane order.  kResidualRows rows per workgroup, blockIdx.y the level of a stack; a pixel's left and right values are read
// once for the three channels.  k_residual_total: one wave per level adds the rows the same way.  No atomics: the same bytes every run.
constexpr int kResidualRows = 4;
template <int L>
__global__ __launch_bounds__(64 * kResidualRows) void k_residual_rows(ResidualArgs a)
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
__global__ __launch_bounds__(64) void k_residual_total(ResidualArgs a, double *__restrict__ sums)
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
    const dim3 grid((a.H + kResidualRows - 1) / kResidualRows, a.levels);
    if (in == kInPlanes) {
        const Rows rows = k_residual_rows<kInPlanes>;
        UGSM_LAUNCH(rows, grid, dim3(64 * kResidualRows), 0, st, a);
    } else {
        const bool words = input_words_aligned(static_cast<const uint8_t *>(a.L), a.stride, nullptr) &&
                           input_words_aligned(static_cast<const uint8_t *>(a.R), a.stride, nullptr);
        with_layout(input_layout(in, words), [&](auto layout) {
            const Rows rows = k_residual_rows<decltype(layout)::value>;
            UGSM_LAUNCH(rows, grid, dim3(64 * kResidualRows), 0, st, a);
        });
    }
    UGSM_LAUNCH(k_residual_total, dim3(a.levels), dim3(64), 0, st, a, sums);
}

}  // namespace ugsm
