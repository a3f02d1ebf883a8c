// ugsm_tri.hpp -- SURVEY 8f row f-1, the device functions that the plane / depth kernels (ugsm_kernels_depth.hip) and the cloud kernels
// (ugsm_kernels_cloud.hip) share: the closed form of a correspondence's X, Y, Z (tri_point, under a lens tri_point_lens), where a pixel's
// (dx, dy, conf) comes from (PlaneSrc, FrameSrc), a pixel's point (tri_at, tri_of), its colour word, the compact clouds' filter and the
// resized map's point (cubic_tap, resized_point); and, for the two files' launchers, proj() and UGSM_LAUNCH_LENS.  Device code: .hip files only.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#pragma once

#include "ugsm_device.hpp"
#include "ugsm_launch.hpp"
#include "ugsm_lens.hpp"

namespace ugsm {

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

// ... under a lens (ugsm_set_lens; ugsm_lens.hpp): the two positions undistorted, each by its own camera, just before the closed form.  The
// caller keeps the distorted (x1, y1): the colour, the fovea forms' (int)x1 and the coverage rule are about pixels.
__device__ __forceinline__ void tri_point_lens(const Lens &ln, float x1, float y1, float x2, float y2, const double *P1, const double *P2, float &X,
                                               float &Y, float &Z)
{
    float u1, v1, u2, v2;
    undistort_point(ln.cam[0], ln.iterations, x1, y1, u1, v1);
    undistort_point(ln.cam[1], ln.iterations, x2, y2, u2, v2);
    tri_point(u1, v1, u2, v2, P1, P2, X, Y, Z);
}
// A kernel that honours the lens is the same kernel with one more argument, the Lens by value behind its last (template parameter pack
// LensArg: empty, or Lens); the instances without it keep the argument list and the code they had.  L below: the launch has a lens, and ln
// points at it (else null and not read).
__device__ __forceinline__ const Lens *lens_of() { return nullptr; }
__device__ __forceinline__ const Lens *lens_of(const Lens &ln) { return &ln; }

// Where a pixel's (dx, dy, conf) comes from -- template parameter Src of tri_at, resized_point, depth_run and depth_resized.  PlaneSrc, the
// default: the planes of CloudArgs, read where each routine has always read them; its instances are the code they were (tools/isa_dump.py
// --diff).  FrameSrc (k_triangulate's frame forms): the value ugsm_reconstruct_full[_multi] would have put at frame pixel (x, y), by descent through the
// fovea stack as k_restrict_stack walks it.  At level l < F-1 the site lies inside a window when 0 <= x - ox[l] < fw && 0 <= y - oy[l] < fh
// (Table: every window is tried and the highest-numbered one that holds the site supplies the value); else it moves to
// tex_index(((float)x + 0.5f) / s, w[l + 1]), the same in y; level F-1 holds every site and is stack 0's.  The level's sizes and the windows'
// origins are uniform (scalar loads by a uniform index); a lane that has found its level stops moving, and the wave leaves the loop when every
// lane has.  Then one multiplication by s per level descended, every channel, each product rounded on its own.  A thread walks the N pixels of
// its run side by side, so that their loads go out together.  Nothing is read outside the stacks: a window test precedes every read of a
// level below F-1 and tex_index clamps to level F-1's own size (the launcher checks that every window lies inside its level).  A disparity
// never indexes anything here: NaN, infinite and huge values pass through.
struct PlaneSrc {
    static constexpr bool kPlanes = true;
};
// tex_index(((float)c + 0.5f) / s, n) for c >= 0, s = (float)1.41421356: a descent's step, two of them per pixel and level, and the IEEE
// division is what the step costs.  q = a * RN(1 / s) lies within 1.5 q 2^-23 of the quotient's exact value and of its rounded one, so
// wherever q is further than q 2^-21 from both neighbouring integers, floor(q) IS floor(RN(a / s)); elsewhere (3 columns in a thousand of a
// 16 MP frame; every q from 2^21 on) the division itself is made, behind a branch a wave skips when no lane needs it.  Every operation is a
// binary32 one with the same result on the host: the equality has been checked there for every c below 2^28.
__device__ __forceinline__ int frame_down(int c, int n)
{
    const float s = (float)1.41421356, rs = 1.0f / s;
    const float a = (float)c + 0.5f;
    const float q = a * rs;
    float f = floorf(q);
    const float fr = q - f, m = q * 0x1p-21f;
    if (!(fr > m && fr < 1.0f - m)) f = floorf(a / s);
    return f > (float)(n - 1) ? n - 1 : (int)f;  // (f >= 0: tex_index's other clamp never acts)
}
template <bool Table>
struct FrameSrc {
    static constexpr bool kPlanes = false;
    const float *sx, *sy, *sc;  // stack 0's planes; sc null: no confidence (0.0f)
    const DepthFrame *f;
    template <int N>
    __device__ __forceinline__ void fetch(const int (&px)[N], const int (&py)[N], float (&dx)[N], float (&dy)[N], float (&cf)[N]) const
    {
        const float s = (float)1.41421356;
        const DepthFrame &fr = *f;
        const int fn = fr.fw * fr.fh, last = fr.F - 1;
        int x[N], y[N], depth[N], at[N];
        long long sh[N];
        bool found[N];
#pragma unroll
        for (int e = 0; e < N; e++) {
            x[e] = px[e];
            y[e] = py[e];
            depth[e] = last;
            at[e] = 0;
            sh[e] = 0;
            found[e] = false;
        }
        for (int l = 0; l < last; l++) {  // (uniform)
            bool hit[N];
#pragma unroll
            for (int e = 0; e < N; e++) hit[e] = false;
            const int nw = Table ? fr.n : 1;
            for (int j = 0; j < nw; j++) {
                const FrameWindow &w = Table ? fr.table[j] : fr.win;
                const int ox = w.ox[l], oy = w.oy[l];
                const long long st = w.stack;
#pragma unroll
                for (int e = 0; e < N; e++) {
                    const int fx = x[e] - ox, fy = y[e] - oy;
                    if (!found[e] && fx >= 0 && fx < fr.fw && fy >= 0 && fy < fr.fh) {
                        hit[e] = true;
                        at[e] = l * fn + fy * fr.fw + fx;
                        sh[e] = st;
                    }
                }
            }
            bool open = false;
#pragma unroll
            for (int e = 0; e < N; e++) {
                if (hit[e]) {
                    found[e] = true;
                    depth[e] = l;
                } else if (!found[e]) {
                    x[e] = frame_down(x[e], fr.w[l + 1]);
                    open = true;
                }
            }
            // rows move whether found or not (a found lane no longer reads its row), so that a pixel in its left neighbour's row takes that
            // neighbour's: a run lies in one row or two
#pragma unroll
            for (int e = 0; e < N; e++) {
                if (e > 0 && py[e] == py[e - 1]) y[e] = y[e - 1];
                else y[e] = frame_down(y[e], fr.h[l + 1]);
            }
            if (__ballot(open) == 0) break;
        }
#pragma unroll
        for (int e = 0; e < N; e++) {
            if (!found[e]) at[e] = last * fn + y[e] * fr.fw + x[e];
            dx[e] = shifted(sx, sh[e])[at[e]];
            dy[e] = shifted(sy, sh[e])[at[e]];
            cf[e] = sc ? shifted(sc, sh[e])[at[e]] : 0.0f;
        }
        for (int j = 0; j < last; j++) {  // (uniform; a lane multiplies while j < its depth)
#pragma unroll
            for (int e = 0; e < N; e++) {
                if (j < depth[e]) {
                    dx[e] = s * dx[e];
                    dy[e] = s * dy[e];
                    cf[e] = s * cf[e];
                }
            }
        }
    }
    __device__ __forceinline__ void fetch1(int x, int y, float &dx, float &dy, float &cf) const
    {
        const int px[1] = {x}, py[1] = {y};
        float vx[1], vy[1], vc[1];
        fetch<1>(px, py, vx, vy, vc);
        dx = vx[0];
        dy = vy[0];
        cf = vc[0];
    }
};

// X, Y, Z of pixel (ii, jj) of the planes, from the same operands as the plane kernels (bit-identical to them); (x1, y1) the pixel in the
// full-resolution frame.
template <bool Fovea, bool L = false, class Src = PlaneSrc>
__device__ __forceinline__ void tri_at(const CloudArgs &a, const Proj &P1q, const Proj &P2q, int ii, int jj, float &x1, float &y1, float &X,
                                       float &Y, float &Z, const Lens *ln = nullptr, const Src *src = nullptr)
{
    const size_t at = (size_t)jj * a.pw + ii;
    float x2, y2;
    if constexpr (!Src::kPlanes) {  // the field form on the source's value
        static_assert(!Fovea, "a source other than the planes gives a full-resolution field");
        float ddx, ddy, unused;
        src->fetch1(ii, jj, ddx, ddy, unused);
        x1 = ii;
        y1 = jj;
        x2 = ii + ddx;
        y2 = jj + ddy;
    } else if (Fovea) {  // as k_triangulate_fovea
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
    if constexpr (L) tri_point_lens(*ln, x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
    else tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
}
// ... from the pixel's disparity (ddx, ddy), for a caller that has loaded it already: the depth image's runs, which read eight pixels'
// disparities with 16-byte loads.  The operands are tri_at's, line for line, with the loaded value where tri_at reads the plane; the two stay
// apart because tri_at written as a call of this one moved the register allocation of k_cloud_fovea<kTriResized> (tools/isa_dump.py --diff),
// and tests/test_gpu_depth.py holds them to the same bits.
template <bool Fovea, bool L = false>
__device__ __forceinline__ void tri_of(const CloudArgs &a, const Proj &P1q, const Proj &P2q, int ii, int jj, float ddx, float ddy, float &x1, float &y1,
                                       float &X, float &Y, float &Z, const Lens *ln = nullptr)
{
    float x2, y2;
    if (Fovea) {  // as k_triangulate_fovea
        x1 = (float)a.left_margin + (float)ii * a.scale;
        y1 = (float)a.upper_margin + (float)jj * a.scale;
        const int sx = (int)(ii + ddx);
        const int sy = (int)(jj + ddy);
        x2 = (float)a.left_margin + (float)sx * a.scale;
        y2 = (float)a.upper_margin + (float)sy * a.scale;
    } else {      // as k_triangulate
        x1 = ii;
        y1 = jj;
        x2 = ii + ddx;
        y2 = jj + ddy;
    }
    if constexpr (L) tri_point_lens(*ln, x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
    else tri_point(x1, y1, x2, y2, P1q.m, P2q.m, X, Y, Z);
}

// The colour word of pixel cx of an image row in any input format (UGSM_INPUT_*; fmt is uniform): R << 16 | G << 8 | B of the pixel's
// conversion to rgb8.  The three- and four-byte formats read bytes 0, 1, 2 at fixed offsets (two loads) and select the channel order.
// Not a switch over the formats: that puts the colour loads and their waits ahead of the arithmetic, and the resized clouds' short
// launches take up to a sixth longer.
// A float sample as the byte of the colour word: NaN or v <= 0 -> 0, v >= 255 -> 255, else (uint8_t)(v + 0.5f) -- an integer-valued sample gives
// the byte an 8-bit image would hold.
__device__ __forceinline__ unsigned colour_byte(float v) { return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (unsigned)(v + 0.5f)); }
__device__ __forceinline__ unsigned colour_word(const uint8_t *row, int cx, int fmt)
{
    if (fmt == kInMono32F) return colour_byte(reinterpret_cast<const float *>(row)[cx]) * 0x010101u;
    if (fmt == kInRGB32F) {
        const float *const q = reinterpret_cast<const float *>(row) + (size_t)3 * cx;
        return colour_byte(q[0]) << 16 | colour_byte(q[1]) << 8 | colour_byte(q[2]);
    }
    if (fmt == kInMono8) return (unsigned)row[cx] * 0x010101u;
    const bool swap = fmt == kInBGR8 || fmt == kInBGRA8;
    const uint8_t *p = row + (size_t)((fmt == kInRGBA8 || fmt == kInBGRA8) ? 4 : 3) * cx;
    const unsigned c0 = p[0], c1 = p[1], c2 = p[2];
    return (swap ? c2 : c0) << 16 | c1 << 8 | (swap ? c0 : c2);
}

// the colour word of full-resolution pixel (cx, cy); the foveated kernels clamp it to the image (the reference reads whatever lies there):
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

// SURVEY 8f row f-1, the resized cloud: getPointCloud.cpp doReconstruction_resized (:724-800) / doReconstructionFOV_resized (:802-884),
// cv::resize(range_map, res, Size(pw * f, ph * f), 0, 0, INTER_CUBIC) of the Z plane, then one point per pixel (ii, jj) of the resized
// map, in the same column-major order.  The Z plane is never written: each point evaluates the 16 Z of its 4 x 4 footprint with tri_at
// (k_triangulate's Z, bit for bit) and resizes them in OpenCV's float order (resizeGeneric_ with HResizeCubic / VResizeCubic on CV_32F):
//   taps   fx = (float)((dx + 0.5) * scale_x - 0.5) with scale_x = 1. / ((double)dw / pw) in double, sx = floor(fx), fx -= sx in float;
//          columns sx-1 .. sx+2 and rows sy-1 .. sy+2 clamped to the plane (replicate border);
//   coeffs interpolateCubic, A = -0.75f, in float; c3 = 1 - c0 - c1 - c2;
//   sums   each source row ((S0*c0 + S1*c1) + S2*c2) + S3*c3 left to right, from +0.0f on the border columns (sx < 1 or sx + 2 >= pw:
//          HResizeCubic's clamped loop accumulates from 0, which only turns a -0.0f sum into +0.0f); then ((R0*b0 + R1*b1) + R2*b2) + R3*b3;
//          every product rounded on its own (the library builds with -ffp-contract=off).  NaN and inf propagate (0 * inf is NaN).
//   same   cv::resize copies the plane when the size does not change (factor 1), so there Z is the pixel's own Z.
// X, Y are get3DPoint's at xx = (int)((float)ii / f), yy = (int)((float)jj / f) (IEEE float division) -- the reference's registration:
// the cubic's centre lies near ii / f + (1 / f - 1) / 2, two pixels further on at f = 0.2, and it is kept.  The colour is the left
// image's at (xx, yy); the foveated kernel reads it there too, in the full image's top-left corner (:864-867), unless colour_mapped asks
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

// Rec (the depth image's use): the record is written whether or not there is a colour to read -- (X, Y, Z, 0) -- so that rec.z hands the
// resized map's Z to a caller that keeps nothing else
template <bool Fovea, bool Colour, bool Rec = Colour, bool L = false, class Src = PlaneSrc>
__device__ __forceinline__ bool resized_point(const CloudArgs &a, const CloudResize &rz, const Proj &P1q, const Proj &P2q, int ii, int jj,
                                              float4 &rec, const Lens *ln = nullptr, const Src *src = nullptr)
{
    // (ii < (int)(pw * f) keeps ii / f below pw; the clamp never acts)
    const int xx = min((int)((float)ii / rz.factor), a.pw - 1);
    const int yy = min((int)((float)jj / rz.factor), a.ph - 1);
    float x1, y1, X, Y, Z;
    tri_at<Fovea, L, Src>(a, P1q, P2q, xx, yy, x1, y1, X, Y, Z, ln, src);
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
                tri_at<Fovea, L, Src>(a, P1q, P2q, min(max(sx - 1 + k, 0), a.pw - 1), ty, u1, u2, u3, u4, s[k], ln, src);
            }
            const float p0 = s[0] * cx[0];
            const float h = (((border ? 0.0f + p0 : p0) + s[1] * cx[1]) + s[2] * cx[2]) + s[3] * cx[3];
            v = r == 0 ? h * cy[0] : v + h * cy[r];
        }
        Z = v;
    }
    if (Rec) rec = make_float4(X, Y, Z, __uint_as_float(word));
    return cloud_keep(a, (size_t)yy * a.pw + xx, X, Y, Z);
}

// a 3x4 projection matrix as the kernels take it
inline Proj proj(const double *P)
{
    Proj q;
    for (int k = 0; k < 12; k++) q.m[k] = P[k];
    return q;
}

// Every launcher of ugsm_kernels_depth.hip picks the instance from its `lens` (null: none): the same grid and arguments, the Lens by value behind them.
#define UGSM_LAUNCH_LENS(lens, plain, with_lens, grid, st, ...)                                  \
    do {                                                                                       \
        if (lens) UGSM_LAUNCH(with_lens, grid, dim3(256), 0, st, __VA_ARGS__, *(lens));        \
        else UGSM_LAUNCH(plain, grid, dim3(256), 0, st, __VA_ARGS__);                          \
    } while (0)

}  // namespace ugsm
