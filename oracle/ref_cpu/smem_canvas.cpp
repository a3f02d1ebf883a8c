/*
 * smem_canvas.cpp -- linked into oracle/_ref/ref_driver only.  TEST INFRASTRUCTURE ONLY.  The one place that resolves deviations
 * U2 / U3 for the reference's host driver.
 *
 * The reference's two shared-memory convolutions are defined only where the width is a multiple of 128 and the height a multiple of
 * 64; elsewhere their unguarded loads read the next row or past the buffer and their stores pass its end.  For the driver the stage
 * file is compiled with its two entry points renamed (-DconvolutionRowsGPU=ref_convolutionRowsGPU, likewise Columns), and the names
 * the host driver calls are the wrappers below: the renamed function on a zero canvas of such a size with the image in its top left
 * corner, and the image's part of the result copied back -- what RefStages._smem (tests/ref_stages.py) does in numpy.
 */
#include <cstring>
#include <vector>

extern "C" void ref_convolutionRowsGPU(float *dst, float *src, int w, int h);
extern "C" void ref_convolutionColumnsGPU(float *dst, float *src, int w, int h);

static int up(int n, int m) { return (n + m - 1) / m * m; }

static void on_canvas(void (*conv)(float *, float *, int, int), float *dst, const float *src, int W, int H)
{
    const int cw = up(W, 128), ch = up(H, 64);
    std::vector<float> in((size_t)cw * ch, 0.0f), out((size_t)cw * ch, 0.0f);
    for (int y = 0; y < H; y++) std::memcpy(&in[(size_t)y * cw], src + (size_t)y * W, (size_t)W * sizeof(float));
    conv(out.data(), in.data(), cw, ch);
    for (int y = 0; y < H; y++) std::memcpy(dst + (size_t)y * W, &out[(size_t)y * cw], (size_t)W * sizeof(float));
}

extern "C" void convolutionRowsGPU(float *dst, float *src, int w, int h) { on_canvas(ref_convolutionRowsGPU, dst, src, w, h); }
extern "C" void convolutionColumnsGPU(float *dst, float *src, int w, int h) { on_canvas(ref_convolutionColumnsGPU, dst, src, w, h); }
