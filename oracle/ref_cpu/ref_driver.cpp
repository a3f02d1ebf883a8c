/*
 * ref_driver.cpp -- the main() of oracle/_ref/ref_driver: the reference's host driver (MatchGPULib.cpp) and stage file (MatchLib.cu),
 * compiled for the CPU, called on raw files.  TEST INFRASTRUCTURE ONLY; this file is the project's, the class it calls is the
 * reference's, compiled from where the checkout lies (oracle/Makefile ref-driver).
 *
 * It is a program of its own, run as a child process, because the reference prints to stdout all the time, leaks most of what it
 * allocates and ends every call with cudaDeviceReset.  Images are rgb8, W * H * 3 bytes without padding; planes are float32, W * H each.
 *
 *   ref_driver full    W H left.rgb right.rgb out       match(L, R, 0): 3 planes
 *   ref_driver fovea   W H left.rgb right.rgb out       match(L, R, 1): 3 planes (hierarchicalDisparity of the stack)
 *   ref_driver stack   W H left.rgb right.rgb out out2  setFoveated(1), initStack, matchStackPyramid: levels 0 .. foveatelevel - 1, 3 planes
 *                                                       of fovH * fovW each, to `out`; hierarchicalDisparity of that stack to `out2`
 *   ref_driver pyramid W H left.rgb out                 the planes as match() makes them, gaussiankernel, setConvolutionKernel,
 *                                                       CreatePyramidFromImage: levels 0 .. MAX_LEVEL - 1, 3 planes each
 *   ref_driver taps    out                              gaussiankernel: 5 floats
 *   ref_driver warp    W H right.rgb field out          warpRightImage(planes of right, 3 planes read from `field`): 3 planes
 *
 * Every mode that has sizes of its own also writes them as text to `out`.dims ("w h" per level), so that the caller never has to
 * guess how to cut the file.  The class's own constants are what runs: MAX_LEVEL 14 and, with argc < 3, foveatelevel 7.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "MatchGPULib.h"
#include "MatchLib_common.h"

static std::vector<unsigned char> read_bytes(const char *path, size_t n)
{
    std::vector<unsigned char> b(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(b.data(), 1, n, f) != n || std::fgetc(f) != EOF) {
        std::fprintf(stderr, "ref_driver: %s does not hold exactly %zu bytes\n", path, n);
        std::exit(2);
    }
    std::fclose(f);
    return b;
}

struct Out {
    FILE *f, *dims;
    explicit Out(const char *path) : f(std::fopen(path, "wb")), dims(std::fopen((std::string(path) + ".dims").c_str(), "w"))
    {
        if (!f || !dims) {
            std::fprintf(stderr, "ref_driver: cannot write %s\n", path);
            std::exit(2);
        }
    }
    void planes(float **p, int n, int w, int h)
    {
        for (int k = 0; k < n; k++)
            if (std::fwrite(p[k], sizeof(float), (size_t)w * h, f) != (size_t)w * h) std::exit(2);
        std::fprintf(dims, "%d %d\n", w, h);
    }
    ~Out()
    {
        if (std::fclose(f) || std::fclose(dims)) std::exit(2);
    }
};

static cv_bridge::CvImagePtr image(std::vector<unsigned char> &bytes, int W, int H)
{
    auto p = std::make_shared<cv_bridge::CvImage>();
    p->image.data = bytes.data();
    p->image.rows = H;
    p->image.cols = W;
    p->image.step = (size_t)W * 3;
    return p;
}

/* three float planes of an rgb8 image, plane k = byte k of every pixel (what every entry point of the class starts with) */
static std::vector<std::vector<float>> to_planes(const std::vector<unsigned char> &rgb, int W, int H)
{
    std::vector<std::vector<float>> pl(3, std::vector<float>((size_t)W * H));
    for (int k = 0; k < 3; k++)
        for (size_t i = 0; i < (size_t)W * H; i++) pl[k][i] = (float)rgb[i * 3 + k];
    return pl;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: ref_driver MODE ... (see ref_driver.cpp)\n");
        return 2;
    }
    const std::string mode = argv[1];
    char name[] = "ref_driver";
    char *cargv[] = {name, nullptr};
    MatchGPULib m(1, cargv); /* argc < 3: foveatelevel = 7 */

    if (mode == "taps" && argc == 3) {
        float k[KERNEL_LENGTH];
        m.gaussiankernel(k);
        FILE *f = std::fopen(argv[2], "wb");
        return (f && std::fwrite(k, sizeof(float), KERNEL_LENGTH, f) == KERNEL_LENGTH && !std::fclose(f)) ? 0 : 2;
    }
    if (argc < 6) return 2;
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    if (W < 1 || H < 1) return 2;
    const size_t nimg = (size_t)W * H * 3;

    if ((mode == "full" || mode == "fovea") && argc == 7) {
        auto lb = read_bytes(argv[4], nimg), rb = read_bytes(argv[5], nimg);
        float **d = m.match(image(lb, W, H), image(rb, W, H), mode == "fovea" ? 1 : 0);
        Out(argv[6]).planes(d, 3, W, H);
        return 0;
    }
    if (mode == "stack" && argc == 8) {
        auto lb = read_bytes(argv[4], nimg), rb = read_bytes(argv[5], nimg);
        auto L = image(lb, W, H), R = image(rb, W, H);
        std::vector<float **> lf(MAX_LEVEL), rf(MAX_LEVEL);
        m.setFoveated(1);
        m.initStack(L, R);
        float ***stack = m.matchStackPyramid(L, R, lf.data(), rf.data());
        {
            Out out(argv[6]);
            for (int l = 0; l < m.getFoveateLevel(); l++) out.planes(stack[l], 3, m.getFoveaWidth(), m.getFoveaHeight());
        }
        float **d = m.hierarchicalDisparity(nullptr, stack, 3, W, H); /* its first argument is not used */
        Out(argv[7]).planes(d, 3, W, H);
        return 0;
    }
    if (mode == "pyramid" && argc == 6) {
        auto lb = read_bytes(argv[4], nimg);
        auto pl = to_planes(lb, W, H);
        float *im[3] = {pl[0].data(), pl[1].data(), pl[2].data()};
        float k[KERNEL_LENGTH];
        m.gaussiankernel(k);
        setConvolutionKernel(k);
        float ***pyr = m.CreatePyramidFromImage(im, 3, H, W, k);
        Out out(argv[5]);
        int w = W, h = H;
        for (int l = 0; l < MAX_LEVEL; l++) {
            out.planes(pyr[l], 3, w, h);
            w = w / SCALE; /* the class's own size rule, int = int / double */
            h = h / SCALE;
        }
        return 0;
    }
    if (mode == "warp" && argc == 7) {
        auto rb = read_bytes(argv[4], nimg);
        auto fb = read_bytes(argv[5], (size_t)W * H * 3 * sizeof(float));
        auto pl = to_planes(rb, W, H);
        float *im[3] = {pl[0].data(), pl[1].data(), pl[2].data()};
        float *fld = reinterpret_cast<float *>(fb.data());
        float *d[3] = {fld, fld + (size_t)W * H, fld + (size_t)2 * W * H};
        float **o = m.warpRightImage(im, d, 3, W, H);
        Out(argv[6]).planes(o, 3, W, H);
        return 0;
    }
    std::fprintf(stderr, "ref_driver: unknown mode or wrong number of arguments\n");
    return 2;
}
