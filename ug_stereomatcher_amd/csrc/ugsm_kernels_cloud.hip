// ugsm_kernels_cloud.hip -- SURVEY 8f row f-1: triangulation of a match into X, Y, Z planes and into coloured point clouds.
//
// k_triangulate / k_triangulate_fovea (the X, Y, Z planes and, as their depth forms, the REP 118 depth image -- k_triangulate's frame forms: the
// depth image of the whole frame from a fovea stack), k_cloud / k_cloud_fovea (the coloured cloud and the resized cloud of one field
// or one fovea level), k_cloud_stack (the merged cloud of a whole fovea stack), k_cloud_pairs / k_cloud_stack_pairs (the clouds of the pairs
// of a queue call in one launch), k_cloud_multi (the merged cloud of several windows' stacks).  Every cloud kernel is one tile routine,
// cloud_tile, under a preamble of its own.  HBM-bound.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
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

// =========================================================================================
// SURVEY 8f row f-1, second half: the coloured point cloud, getPointCloud.cpp doReconstructionRGB (:675-722) and
// doReconstructionRGB_FOV (:615-673) -- the node's scalar double loop over the pixels with one push_back per pixel.
// Column ii is the outer loop and row jj the inner one, so the cloud is COLUMN-major while the planes are row-major: record
// (ci, cj) of the sampled grid (ii = ci * s, jj = cj * s) is record ci * hc + cj of the dense cloud.  X, Y, Z are tri_point's, from
// the same operands as k_triangulate computes them (bit-identical); the colour word is R << 16 | G << 8 | B of the left image
// (the node's BGR8 copy, :225, packed at :703-714), i.e. byte0 << 16 | byte1 << 8 | byte2 of the rgb8 buffer, alpha 0.
//
// One workgroup per tile of kCloudTC sampled columns x kCloudTR sampled rows, three phases:
//   A  evaluate: lane (t mod 32) = column, so every read is a row-coalesced run (4-byte dx, dy, conf; rgb bytes); the record
//      (x, y, z, rgb word) goes to LDS at [column][row] and whether it is kept to a byte array;
//   B  one wave per column, lane = row: a ballot of the kept flags gives every kept row its rank in the column's run (dense: every
//      row inside the grid is kept, so the ranks are the rows), and `src` the row of each rank;
//   C  every column's run of the tile is one contiguous block of the output, written with whole 16-byte stores, one wave instruction
//      covering 1 KB of it: 32 records of 32 B (PCL32) or 64 of 16 B (XYZRGB16).
// Compact clouds take two launches.  The count launch (kTriCloudCount) runs A and B and writes each column's kept count per chunk of
// kCloudTR rows, and adds it to the column's and the strip's (the tile column's) totals with integer atomics: order-independent sums,
// deterministic.  The cloud launch (kTriCloud) derives each run's first record from those counts -- the strips to its left, the strip's
// columns to its left, the chunks above it -- and re-evaluates its tile (tri_point is cheap beside a second pass over the output).
// No workgroup waits for another inside a launch.  Records at or past cap are not written; `count` gets the cloud's size.
// =========================================================================================
constexpr int kCloudTC = 32;             // sampled columns per tile
constexpr int kCloudTR = 64;             // sampled rows per tile = lanes of a wave (phase B)
constexpr int kCloudPad = kCloudTR + 1;  // records per column in LDS: column c starts 4c banks further on (phase A stores 32 columns at once)

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

// one sampled point: its record (x, y, z, rgb word as float bits) and whether a compact cloud keeps it
template <bool Fovea, bool Colour, bool L = false>
__device__ __forceinline__ bool cloud_point(const CloudArgs &a, const Proj &P1q, const Proj &P2q, int ii, int jj, float4 &rec, const Lens *ln = nullptr)
{
    float x1, y1, X, Y, Z;
    tri_at<Fovea, L>(a, P1q, P2q, ii, jj, x1, y1, X, Y, Z, ln);
    if (Colour) {  // the foveated kernels: at ((int)mapXcoord(ii), (int)mapYcoord(jj)) of the full-resolution image (:630-640), clamped (colour_at)
        const int cx = Fovea ? min(max((int)x1, 0), a.W - 1) : ii, cy = Fovea ? min(max((int)y1, 0), a.H - 1) : jj;
        rec = make_float4(X, Y, Z, __uint_as_float(colour_word(a.rgb + (size_t)cy * a.stride, cx, a.fmt)));
    }
    return cloud_keep(a, (size_t)jj * a.pw + ii, X, Y, Z);
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

// a 3x4 projection matrix as the kernels take it
static Proj proj(const double *P)
{
    Proj q;
    for (int k = 0; k < 12; k++) q.m[k] = P[k];
    return q;
}

// Every launcher below picks the instance from its `lens` (null: none): the same grid and arguments, the Lens by value behind them.
#define UGSM_LAUNCH_LENS(lens, plain, with_lens, grid, st, ...)                                  \
    do {                                                                                       \
        if (lens) UGSM_LAUNCH(with_lens, grid, dim3(256), 0, st, __VA_ARGS__, *(lens));        \
        else UGSM_LAUNCH(plain, grid, dim3(256), 0, st, __VA_ARGS__);                          \
    } while (0)

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

// The merged cloud of the whole fovea stack (ugsm_point_cloud_fovea_all; kTriStackCount / kTriStack): the same tile over F * strips
// virtual strips, level = strip / strips.  `a` holds the workgroup's level already (its planes and mapping: k_cloud_stack),
// lv is that level's row of the table.  A covered point (sampled column in [cx0, cx1) and row in [cy0, cy1): its footprint lies wholly inside
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
// of stack 0).  What an entry leaves out is a UNION of rectangles of its sampled grid (CloudEntry), so the kernel (k_cloud_multi)
// reduces the entry's list to what the tile needs before the tile runs, 32 lanes = the tile's columns:
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

// What a launch of the tile does (template parameter): the count launch and the cloud launch of the point cloud, of the resized cloud,
// of the fovea stack's merged cloud and of the merged cloud of several windows' stacks.
enum TriForm : int {
    kTriCloudCount = 1, kTriCloud = 2, kTriResizedCount = 3, kTriResized = 4, kTriStackCount = 5, kTriStack = 6, kTriMultiCount = 7, kTriMulti = 8
};

template <bool Fovea, int Form, bool L = false>
__device__ __forceinline__ void cloud_tile(const CloudArgs &a, const CloudResize &rz, const Proj &P1q, const Proj &P2q, const CloudStack *sk = nullptr,
                                           int level = 0, const CloudMulti *mu = nullptr, const MultiTile *mt = nullptr, const Lens *ln = nullptr)
{
    constexpr bool Stack = Form == kTriStackCount || Form == kTriStack;
    constexpr bool Multi = Form == kTriMultiCount || Form == kTriMulti;  // (level: the entry; its early return is the kernel's)
    __shared__ float4 rec[kCloudTC * kCloudPad];
    __shared__ unsigned char kept[kCloudTC * kCloudTR];
    __shared__ unsigned char src[kCloudTC * kCloudTR];
    __shared__ int nrec[kCloudTC];
    __shared__ unsigned pre[kCloudTC + 1];  // compact: [c] the run's first record less the strip's, [kCloudTC] the strip's first record
    // tx: the strip among all of the launch (the stack kernels: F * strips virtual strips); c0: its first column in its level, v0: among
    // the launch's columns (the stack kernels: level * wc + c0, the F * wc virtual columns)
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
                k = resized_point<Fovea, Write, Write, L>(a, rz, P1q, P2q, ci, cj, v, ln);
            else
                k = cloud_point<Fovea, Write, L>(a, P1q, P2q, ci * a.s, cj * a.s, v, ln);
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

// the cloud of one field / of one fovea level; rz: the resized cloud's (unused by the others)
template <int Form, class... LensArg>
__global__ __launch_bounds__(256) void k_cloud(CloudArgs a, Proj P1q, Proj P2q, CloudResize rz, LensArg... lens)
{
    cloud_tile<false, Form, sizeof...(LensArg) != 0>(a, rz, P1q, P2q, nullptr, 0, nullptr, nullptr, lens_of(lens...));
}
template <int Form, class... LensArg>
__global__ __launch_bounds__(256) void k_cloud_fovea(CloudArgs a, Proj P1q, Proj P2q, CloudResize rz, LensArg... lens)
{
    cloud_tile<true, Form, sizeof...(LensArg) != 0>(a, rz, P1q, P2q, nullptr, 0, nullptr, nullptr, lens_of(lens...));
}

// the workgroup's copy of the arguments moved to a level of the stack: the level's planes and mapping
__device__ __forceinline__ void to_level(CloudArgs &a, const CloudLevel &lv)
{
    a.dx += lv.plane;
    a.dy += lv.plane;
    if (a.conf) a.conf += lv.plane;
    a.left_margin = lv.left_margin;
    a.upper_margin = lv.upper_margin;
    a.scale = lv.scale;
}

// the merged cloud of the fovea stack: the workgroup's level from its strip, its copy of the arguments moved there
template <int Form, class... LensArg>
__global__ __launch_bounds__(256) void k_cloud_stack(CloudArgs a, Proj P1q, Proj P2q, CloudStack sk, LensArg... lens)
{
    static_assert(Form == kTriStackCount || Form == kTriStack, "the stack's two launches");
    const int level = blockIdx.x / sk.strips;
    to_level(a, sk.lv[level]);
    cloud_tile<true, Form, sizeof...(LensArg) != 0>(a, CloudResize{}, P1q, P2q, &sk, level, nullptr, nullptr, lens_of(lens...));
}

// The same clouds for the pairs of a queue call in one launch: blockIdx.z = the pair, whose row of the table in
// device memory is what the single-pair kernels take as kernel arguments.  The tile is cloud_tile, untouched: blockIdx.x, blockIdx.y and
// gridDim.x are the single-pair launch's.
template <int Form>
__global__ __launch_bounds__(256) void k_cloud_pairs(const CloudPair *__restrict__ table, Proj P1q, Proj P2q)
{
    static_assert(Form == kTriCloudCount || Form == kTriCloud, "the cloud's two launches, for a call's pairs");
    const CloudArgs a = table[blockIdx.z].a;
    cloud_tile<false, Form>(a, CloudResize{}, P1q, P2q);
}
template <int Form>
__global__ __launch_bounds__(256) void k_cloud_stack_pairs(const CloudPair *__restrict__ table, Proj P1q, Proj P2q)
{
    static_assert(Form == kTriStackCount || Form == kTriStack, "the stack's two launches, for a call's pairs");
    const CloudPair &row = table[blockIdx.z];
    CloudArgs a = row.a;
    const int level = blockIdx.x / row.sk.strips;
    to_level(a, row.sk.lv[level]);
    cloud_tile<true, Form>(a, CloudResize{}, P1q, P2q, &row.sk, level);
}

// The merged cloud of several windows' stacks: the workgroup's entry from its strip; the entry's row of the table in device memory gives its
// planes and mapping into the workgroup's copy of the arguments; its rectangle list is read from the table ONCE, a lane a rectangle, into
// LDS, and reduced from there to the tile's row masks and dense run starts (MultiTile, above cloud_tile).  A tile wholly inside one
// rectangle returns at once (the workgroup that writes the size stays).
template <int Form>
__global__ __launch_bounds__(256) void k_cloud_multi(CloudArgs a, Proj P1q, Proj P2q, CloudMulti mu)
{
    static_assert(Form == kTriMultiCount || Form == kTriMulti, "the two launches of several windows' stacks");
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

// compact: the count launch, then the cloud launch; dense: the cloud launch
template <class Kern, class... Args>
static void launch_cloud(hipStream_t st, bool compact, Kern count, Kern cloud, dim3 grid, const Args &...args)
{
    if (compact) UGSM_LAUNCH(count, grid, dim3(256), 0, st, args...);
    UGSM_LAUNCH(cloud, grid, dim3(256), 0, st, args...);
}

void launch_point_cloud(hipStream_t st, const CloudArgs &args, bool fovea, const double *P1, const double *P2, const CloudResize *rz, const Lens *lens)
{
    const Proj a = proj(P1), b = proj(P2);
    const dim3 grid(cloud_strips(args.wc), args.nchunk);
    const CloudResize r = rz ? *rz : CloudResize{};
    if (lens) {
        using Kern = void (*)(CloudArgs, Proj, Proj, CloudResize, Lens);
        const Kern count = rz ? (fovea ? (Kern)k_cloud_fovea<kTriResizedCount, Lens> : (Kern)k_cloud<kTriResizedCount, Lens>)
                              : (fovea ? (Kern)k_cloud_fovea<kTriCloudCount, Lens> : (Kern)k_cloud<kTriCloudCount, Lens>);
        const Kern cloud = rz ? (fovea ? (Kern)k_cloud_fovea<kTriResized, Lens> : (Kern)k_cloud<kTriResized, Lens>)
                              : (fovea ? (Kern)k_cloud_fovea<kTriCloud, Lens> : (Kern)k_cloud<kTriCloud, Lens>);
        launch_cloud(st, args.compact != 0, count, cloud, grid, args, a, b, r, *lens);
        return;
    }
    using Kern = void (*)(CloudArgs, Proj, Proj, CloudResize);
    const Kern count = rz ? (fovea ? (Kern)k_cloud_fovea<kTriResizedCount> : (Kern)k_cloud<kTriResizedCount>)
                          : (fovea ? (Kern)k_cloud_fovea<kTriCloudCount> : (Kern)k_cloud<kTriCloudCount>);
    const Kern cloud = rz ? (fovea ? (Kern)k_cloud_fovea<kTriResized> : (Kern)k_cloud<kTriResized>)
                          : (fovea ? (Kern)k_cloud_fovea<kTriCloud> : (Kern)k_cloud<kTriCloud>);
    launch_cloud(st, args.compact != 0, count, cloud, grid, args, a, b, r);
}

void launch_point_cloud_stack(hipStream_t st, const CloudArgs &args, const CloudStack &sk, const double *P1, const double *P2, const Lens *lens)
{
    const Proj a = proj(P1), b = proj(P2);
    const dim3 grid(sk.F * sk.strips, args.nchunk);
    if (lens) {
        using Kern = void (*)(CloudArgs, Proj, Proj, CloudStack, Lens);
        const Kern count = k_cloud_stack<kTriStackCount, Lens>, cloud = k_cloud_stack<kTriStack, Lens>;
        launch_cloud(st, args.compact != 0, count, cloud, grid, args, a, b, sk, *lens);
        return;
    }
    using Kern = void (*)(CloudArgs, Proj, Proj, CloudStack);
    const Kern count = k_cloud_stack<kTriStackCount>, cloud = k_cloud_stack<kTriStack>;
    launch_cloud(st, args.compact != 0, count, cloud, grid, args, a, b, sk);
}

void launch_point_cloud_multi(hipStream_t st, const CloudArgs &args, const CloudMulti &mu, const double *P1, const double *P2)
{
    const Proj a = proj(P1), b = proj(P2);
    const dim3 grid(mu.E * cloud_strips(args.wc), args.nchunk);
    using Kern = void (*)(CloudArgs, Proj, Proj, CloudMulti);
    const Kern count = k_cloud_multi<kTriMultiCount>, cloud = k_cloud_multi<kTriMulti>;
    launch_cloud(st, args.compact != 0, count, cloud, grid, args, a, b, mu);
}

void launch_point_cloud_batch(hipStream_t st, const CloudPair *d_table, int n, const CloudPair &shape, bool stack, const double *P1, const double *P2)
{
    const Proj a = proj(P1), b = proj(P2);
    using Kern = void (*)(const CloudPair *, Proj, Proj);
    const Kern count = stack ? (Kern)k_cloud_stack_pairs<kTriStackCount> : (Kern)k_cloud_pairs<kTriCloudCount>;
    const Kern cloud = stack ? (Kern)k_cloud_stack_pairs<kTriStack> : (Kern)k_cloud_pairs<kTriCloud>;
    const dim3 grid(stack ? shape.sk.F * shape.sk.strips : cloud_strips(shape.a.wc), shape.a.nchunk, n);
    launch_cloud(st, shape.a.compact != 0, count, cloud, grid, d_table, a, b);
}

}  // namespace ugsm
