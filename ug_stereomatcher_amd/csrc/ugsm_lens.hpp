// ugsm_lens.hpp -- lens distortion (plumb_bob D) of a correspondence's two pixel positions, stated once for the kernels of
// ugsm_kernels_depth.hip and ugsm_kernels_cloud.hip (through ugsm_tri.hpp) and for the host entry point ugsm_undistort_points (include/ugsm.h, "lens distortion").
//
// The fixed-point iteration of OpenCV's undistortPoints with R = I, P = K for a camera K (fx, fy, cx, cy; skew ignored) and
// D = (k1, k2, p1, p2, k3): the pixel coordinate is binary32, every operation below is binary64 and rounded on its own (the library builds
// with -ffp-contract=off), division is IEEE, and the result is rounded to binary32 once.  With all five coefficients zero the result is the
// input, bit for bit, for every coordinate a frame can hold (the binary64 round trip errs by 1e-12 px); zero D is not special-cased.
#pragma once

#include <hip/hip_runtime.h>

namespace ugsm {

struct LensCam {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3;
};
// What a kernel that honours the lens takes by value beside its two Proj: camera 1 undistorts (x1, y1), camera 2 (x2, y2).
struct Lens {
    LensCam cam[2];
    int iterations;  // 1 .. 32, the same for every point of a launch
};

__host__ __device__ inline void undistort_point(const LensCam &c, int iterations, float u, float v, float &uo, float &vo)
{
    const double x0 = ((double)u - c.cx) / c.fx, y0 = ((double)v - c.cy) / c.fy;
    double x = x0, y = y0;
#pragma nounroll
    for (int it = 0; it < iterations; it++) {
        const double r2 = x * x + y * y;
        const double ic = 1.0 / (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        const double dX = 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
        const double dY = c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
        x = (x0 - dX) * ic;
        y = (y0 - dY) * ic;
    }
    uo = (float)(x * c.fx + c.cx);
    vo = (float)(y * c.fy + c.cy);
}

}  // namespace ugsm
