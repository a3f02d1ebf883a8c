// MatchGPULib_ugsm.hpp -- source-compatible C++ shim of the reference's MatchGPULib class
// (/root/reference/src/gpu_matcher/MatchGPULib.h:6-47) over the C-ABI of include/ugsm.h.
//
// The node's call sites (UG_GPU_matcher.cpp:160-181,423,530-535,645) compile unchanged against
// this header: same constructor, same method names, same return layouts (malloc'd float** /
// float***, freed by the caller exactly as the node already does, :414-418,487-489,636-640,689-691).
// The image argument is templated on "something with ->image.{rows,cols,step,data}", i.e.
// cv_bridge::CvImagePtr in the node, or MatchGPULib::view(msg) of a message the library reads as it
// is (setInputFormat); the header itself needs neither OpenCV nor ROS.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>

#include "ugsm.h"

class MatchGPULib {
public:
    bool foveatedmatching;
    int foveatelevel;
    int fovH;
    int fovW;
    int frames_in_flight = 1;  // (not in the reference) pairs the pipelined calls keep outstanding; "-inflight=N"

    // MatchGPULib.cpp:251-265: "-device=N" anywhere in argv, argv[2] = number of fovea levels (7)
    MatchGPULib(int argc, char **argv) : foveatedmatching(false), foveatelevel(7), fovH(0), fovW(0), ctx_(nullptr)
    {
        ugsm_config cfg;
        ugsm_default_config(&cfg);
        int lr_modes = -1;  // "-lrmodes=N" not given: the context's default, (lr_check_threshold, UGSM_LR_FULL)
        for (int i = 1; i < argc; i++) {
            if (argv[i] && std::strncmp(argv[i], "-device=", 8) == 0) cfg.device = std::atoi(argv[i] + 8);
            // not in the reference: "-lrcheck=TAU" switches the optional LR-consistency check on (ugsm_config.lr_check_threshold;
            // full mode only; off by default, and the results are the reference's only while it is off)
            if (argv[i] && std::strncmp(argv[i], "-lrcheck=", 9) == 0) cfg.lr_check_threshold = (float)std::atof(argv[i] + 9);
            // ... and "-lrmodes=N" names the calls that apply it (UGSM_LR_FULL = 1, UGSM_LR_FOVEATED = 2, both = 3; ugsm_set_lr_check):
            // with 2 or 3 the foveated stacks are checked level by level, both directions in one lockstep call.  Without it: full mode only
            if (argv[i] && std::strncmp(argv[i], "-lrmodes=", 9) == 0) lr_modes = std::atoi(argv[i] + 9);
            // not in the reference: "-inflight=N" sizes the context for the pipelined calls below (N pairs outstanding in the library's
            // queue: min(N, 4) slots, ceil(N / slots) pairs per call at most); 1 = the reference's one blocking call at a time
            if (argv[i] && std::strncmp(argv[i], "-inflight=", 10) == 0) frames_in_flight = std::atoi(argv[i] + 10);
        }
        if (frames_in_flight < 1) frames_in_flight = 1;
        cfg.slots = frames_in_flight < 4 ? frames_in_flight : 4;
        cfg.batch = (frames_in_flight + cfg.slots - 1) / cfg.slots;
        if (cfg.batch > 8) cfg.batch = 8;
        if (argc > 2) foveatelevel = std::atoi(argv[2]);
        cfg.fovea_levels = foveatelevel;
        levels_ = cfg.levels;
        const int st = ugsm_create(&cfg, &ctx_);
        if (st != UGSM_OK) throw std::runtime_error(std::string("ugsm_create: ") + ugsm_status_string(st));
        if (lr_modes >= 0) {
            const int sl = ugsm_set_lr_check(ctx_, cfg.lr_check_threshold, lr_modes);
            if (sl != UGSM_OK) {
                ugsm_destroy(ctx_);
                throw std::runtime_error(std::string("ugsm_set_lr_check (-lrmodes): ") + ugsm_status_string(sl));
            }
        }
    }
    ~MatchGPULib() { ugsm_destroy(ctx_); }
    MatchGPULib(const MatchGPULib &) = delete;
    MatchGPULib &operator=(const MatchGPULib &) = delete;

    int getFoveaWidth() { return fovW; }
    int getFoveaHeight() { return fovH; }
    int getFoveateLevel() { return foveatelevel; }
    void setFoveaWidth(int rows) { fovW = rows; }
    void setFoveaHeight(int cols) { fovH = cols; }
    void setFoveated(int fov) { foveatedmatching = fov; }

    // (not in the reference) the byte layout of the images the next calls hand over: UGSM_INPUT_RGB8 (what cv_bridge's toCvCopy(.., RGB8)
    // gives), or ugsm_input_format_from_encoding(msg.encoding) for a message read in place (view() below): the 8-bit encodings rgb8, bgr8,
    // rgba8, bgra8, mono8, and 32FC3 / 32FC1 (UGSM_INPUT_RGB32F / UGSM_INPUT_MONO32F: data 4-byte aligned, step a multiple of 4).
    // UGSM_ERR_BAD_ARG for an unknown one.
    int setInputFormat(int format) { return ugsm_set_input_format(ctx_, format); }
    // (not in the reference) the LR check of a live node: the threshold (0 = off) and the calls that apply it (UGSM_LR_FULL | UGSM_LR_FOVEATED).
    // UGSM_ERR_STATE while pipelined pairs are outstanding.
    int setLRCheck(float tau, int modes) { return ugsm_set_lr_check(ctx_, tau, modes); }
    // (not in the reference, whose cloud node reads K and D and never uses them) the plumb_bob lens of the two cameras, as the two
    // sensor_msgs::CameraInfo hold it -- setLens(infoL.K.data(), infoL.D.data(), infoR.K.data(), infoR.D.data()) with D of five entries --:
    // depthImage, depthImageStack and every cloud taken from context() undistort the two positions of each correspondence before they
    // triangulate (include/ugsm.h, "lens distortion").  iterations 0 = 5.  The queue's clouds (ugsm_enqueue_*_cloud*) refuse while a lens
    // is set, so a node that publishes its cloud from the queue leaves it off.
    int setLens(const double *K1, const double *D1, const double *K2, const double *D2, int iterations = 0)
    {
        return ugsm_set_lens(ctx_, K1, D1, K2, D2, iterations);
    }
    int clearLens() { return ugsm_set_lens(ctx_, nullptr, nullptr, nullptr, nullptr, 0); }

    // (not in the reference) a sensor_msgs::Image -- anything with height, width, step, data and header -- read in place: what the templated
    // calls below take instead of a cv_bridge copy (->image.{rows,cols,step,data}, ->header).  The message must outlive the call.
    template <class Header>
    struct ImageView {
        struct {
            int rows, cols;
            size_t step;
            const uint8_t *data;
        } image;
        Header header;
        const ImageView *operator->() const { return this; }
    };
    template <class Msg>
    static ImageView<decltype(Msg::header)> view(const Msg &m)
    {
        ImageView<decltype(Msg::header)> v;
        v.image.rows = (int)m.height;
        v.image.cols = (int)m.width;
        v.image.step = (size_t)m.step;
        v.image.data = m.data.data();
        v.header = m.header;
        return v;
    }

    // MatchGPULib.cpp:406-426
    template <class ImgPtr>
    int initStack(ImgPtr L, ImgPtr /*R*/)
    {
        return ugsm_fovea_dims(L->image.cols, L->image.rows, 14, foveatelevel, &fovW, &fovH) == UGSM_OK ? 0 : -1;
    }

    // MatchGPULib.cpp:303-403 (fov == 0).  Returns finDisp[3][rows*cols]; nullptr on failure
    // (the reference exit()s instead).
    template <class ImgPtr>
    float **match(ImgPtr L, ImgPtr R, int fov)
    {
        foveatedmatching = fov;
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return nullptr;
        float **fin = alloc_planes(3, (size_t)W * H);
        // fov == 1: foveated matching + hierarchicalDisparity (MatchGPULib.cpp:354-360)
        const int st = fov == 1 ? ugsm_match_foveated_full(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, 0, 0, fin[0], fin[1], fin[2])
                                : ugsm_match_full(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, fin[0], fin[1], fin[2]);
        if (st != UGSM_OK) return fail(fin, 3, st);
        return fin;
    }

    // (not in the reference) match(L, R, 0) with the LR check at threshold tau for this call alone (ugsm_match_full_checked: both directions in
    // one lockstep call; the context's setLRCheck setting is neither read nor changed).  Returns the left camera's checked finDisp and, where
    // `back` is given, the right camera's in *back, malloc'd the same way.  tau <= 0 or fov != 0: match(L, R, fov), *back = nullptr.
    template <class ImgPtr>
    float **match(ImgPtr L, ImgPtr R, int fov, float tau, float ***back = nullptr)
    {
        if (back) *back = nullptr;
        if (fov != 0 || !(tau > 0.0f)) return match(L, R, fov);
        foveatedmatching = fov;
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return nullptr;
        float **fin = alloc_planes(3, (size_t)W * H), **bk = back ? alloc_planes(3, (size_t)W * H) : nullptr;
        const int st = ugsm_match_full_checked(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, fin[0], fin[1], fin[2], bk ? bk[0] : nullptr,
                                               bk ? bk[1] : nullptr, bk ? bk[2] : nullptr, tau);
        if (st != UGSM_OK) {
            if (bk) { for (int c = 0; c < 3; c++) std::free(bk[c]); std::free(bk); }
            return fail(fin, 3, st);
        }
        if (back) *back = bk;
        return fin;
    }

    // (not in the reference) match(L, R, 0) started at level start_level from `prior` -- a finDisp[3][rows*cols] of the same size, the previous
    // frame's say -- instead of from the zero seed at the top level (ugsm_match_full_seeded).  Returns a fresh finDisp; the prior stays the caller's.
    template <class ImgPtr>
    float **matchSeeded(ImgPtr L, ImgPtr R, float *const *prior, int start_level)
    {
        foveatedmatching = 0;
        const int W = L->image.cols, H = L->image.rows;
        if (!prior || R->image.cols != W || R->image.rows != H) return nullptr;
        float **fin = alloc_planes(3, (size_t)W * H);
        const int st = ugsm_match_full_seeded(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, prior[0], prior[1], prior[2], start_level,
                                              fin[0], fin[1], fin[2]);
        if (st != UGSM_OK) return fail(fin, 3, st);
        return fin;
    }

    // (not in the reference) match(L, R, 0) in two halves.  matchCoarse stops when level stop_level has finished and returns that level's field,
    // state[3][h*w] of the level's own size (ugsm_level_dims) -- a field at reduced resolution from the full-resolution images; with `full` it also
    // hands out the field's prolongation to the images' size, a finDisp (ugsm_match_full_coarse).  matchFine runs the rest from such a state
    // (ugsm_match_full_fine): with matchCoarse's state of the same pair, match(L, R, 0)'s finDisp bit for bit.  The state stays the caller's.
    template <class ImgPtr>
    float **matchCoarse(ImgPtr L, ImgPtr R, int stop_level, float ***full = nullptr)
    {
        foveatedmatching = 0;
        const int W = L->image.cols, H = L->image.rows;
        int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
        if (full) *full = nullptr;
        if (R->image.cols != W || R->image.rows != H || stop_level < 0 || stop_level >= levels_ || ugsm_level_dims(W, H, levels_, w, h) != UGSM_OK) return nullptr;
        float **state = alloc_planes(3, (size_t)w[stop_level] * h[stop_level]), **fin = full ? alloc_planes(3, (size_t)W * H) : nullptr;
        const int st = ugsm_match_full_coarse(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, stop_level, state[0], state[1], state[2],
                                              fin ? fin[0] : nullptr, fin ? fin[1] : nullptr, fin ? fin[2] : nullptr);
        if (st != UGSM_OK) {
            if (fin) { for (int c = 0; c < 3; c++) std::free(fin[c]); std::free(fin); }
            return fail(state, 3, st);
        }
        if (full) *full = fin;
        return state;
    }
    template <class ImgPtr>
    float **matchFine(ImgPtr L, ImgPtr R, float *const *state, int state_level)
    {
        foveatedmatching = 0;
        const int W = L->image.cols, H = L->image.rows;
        if (!state || R->image.cols != W || R->image.rows != H) return nullptr;
        float **fin = alloc_planes(3, (size_t)W * H);
        const int st = ugsm_match_full_fine(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, state[0], state[1], state[2], state_level,
                                            fin[0], fin[1], fin[2]);
        if (st != UGSM_OK) return fail(fin, 3, st);
        return fin;
    }

    // MatchGPULib.cpp:429-531.  Returns disparity[level][3][fovH*fovW] for level < foveatelevel.
    template <class ImgPtr>
    float ***matchStack(ImgPtr L, ImgPtr R) { return stack(L, R, nullptr, nullptr); }

    // (not in the reference) matchStack for the window at off[2] started at fovea level start_level from `prior_stack` -- a
    // disparity[level][3][fovH*fovW] as matchStack returns it, the previous frame's at the offsets prior_off[2] -- instead of from the zero seed at
    // the top level (ugsm_match_foveated_warm).  Returns a fresh stack; the levels above start_level are the prior carried over; the prior stays
    // the caller's.  A chain of these never refreshes the levels above start_level: run matchStack again now and then.
    template <class ImgPtr>
    float ***matchStackSeeded(ImgPtr L, ImgPtr R, float **const *prior_stack, const int *prior_off, const int *off, int start_level)
    {
        const int W = L->image.cols, H = L->image.rows, F = foveatelevel;
        if (!prior_stack || !prior_off || !off || R->image.cols != W || R->image.rows != H) return nullptr;
        if (ugsm_fovea_dims(W, H, 14, F, &fovW, &fovH) != UGSM_OK) return nullptr;
        const size_t fn = (size_t)fovW * fovH, sn = fn * F;
        float *in = (float *)std::malloc(3 * sn * sizeof(float)), *sh = (float *)std::malloc(3 * sn * sizeof(float));
        for (int k = 0; k < F; k++)
            for (int c = 0; c < 3; c++) std::memcpy(in + c * sn + k * fn, prior_stack[k][c], fn * sizeof(float));
        const int st = ugsm_match_foveated_warm(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, off[0], off[1], in, in + sn, in + 2 * sn,
                                                prior_off[0], prior_off[1], start_level, sh, sh + sn, sh + 2 * sn);
        float ***disp = nullptr;
        if (st == UGSM_OK) {
            disp = (float ***)std::malloc(F * sizeof(float **));
            for (int k = 0; k < F; k++) {
                disp[k] = alloc_planes(3, fn);
                for (int c = 0; c < 3; c++) std::memcpy(disp[k][c], sh + c * sn + k * fn, fn * sizeof(float));
            }
        } else {
            std::fprintf(stderr, "ugsm: %s: %s\n", ugsm_status_string(st), ugsm_last_error(ctx_));
        }
        std::free(in);
        std::free(sh);
        return disp;
    }

    // Several windows of one pair (not in the reference; include/ugsm.h, "several fovea windows on ONE pair"): matchStack for the n offsets
    // (1 <= n <= UGSM_MAX_BATCH) in one call -- pyramids and the coarse levels once, the windows' fine levels in lockstep.  out[k]: the
    // disparity[level][3][fovH*fovW] matchStack returns for (off_x[k], off_y[k]), malloc'd the same way.  False on failure (nothing allocated).
    // tau > 0: the checked call (ugsm_match_foveated_multi_checked) -- stack k is matchStack's at offset k under setLRCheck(tau, 2).
    template <class ImgPtr>
    bool matchStackMulti(ImgPtr L, ImgPtr R, int n, const int *off_x, const int *off_y, float ****out, float tau = 0.0f)
    {
        const int W = L->image.cols, H = L->image.rows, F = foveatelevel;
        if (!out || n < 1 || n > UGSM_MAX_BATCH || R->image.cols != W || R->image.rows != H) return false;
        if (ugsm_fovea_dims(W, H, 14, F, &fovW, &fovH) != UGSM_OK) return false;
        const size_t fn = (size_t)fovW * fovH, sn = fn * F;
        float *sh = (float *)std::malloc((size_t)n * 3 * sn * sizeof(float));
        float *ph[UGSM_MAX_BATCH], *pv[UGSM_MAX_BATCH], *pc[UGSM_MAX_BATCH];
        for (int k = 0; k < n; k++) { ph[k] = sh + (size_t)k * 3 * sn; pv[k] = ph[k] + sn; pc[k] = pv[k] + sn; }
        const int st = tau > 0.0f ? ugsm_match_foveated_multi_checked(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, n, off_x, off_y, ph, pv, pc, tau)
                                  : ugsm_match_foveated_multi(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, n, off_x, off_y, ph, pv, pc);
        if (st != UGSM_OK) { report(st); std::free(sh); return false; }
        for (int k = 0; k < n; k++) {
            out[k] = (float ***)std::malloc(F * sizeof(float **));
            for (int l = 0; l < F; l++) {
                out[k][l] = alloc_planes(3, fn);
                for (int c = 0; c < 3; c++) std::memcpy(out[k][l][c], ph[k] + c * sn + l * fn, fn * sizeof(float));
            }
        }
        std::free(sh);
        return true;
    }

    // MatchGPULib.cpp:534-700.  leftFov/rightFov: caller-allocated [14][3][fovH*fovW] as in
    // UG_GPU_matcher.cpp:169-179; levels < foveatelevel are filled.
    template <class ImgPtr>
    float ***matchStackPyramid(ImgPtr L, ImgPtr R, float ***leftFov, float ***rightFov) { return stack(L, R, leftFov, rightFov); }

    // MatchGPULib.cpp:2589-2701.  foveated[level][channel] = fovW*fovH floats for level < foveatelevel (what
    // matchStack returns); `im` is unused, as in the reference.  Returns 3 malloc'd planes widthInit*heightInit.
    float **hierarchicalDisparity(float ** /*im*/, float ***foveated, int channels, int widthInit, int heightInit)
    {
        if (channels != 3 || !foveated) return nullptr;
        const int F = foveatelevel;
        if (ugsm_fovea_dims(widthInit, heightInit, 14, F, &fovW, &fovH) != UGSM_OK) return nullptr;
        const size_t fn = (size_t)fovW * fovH, sn = fn * F, n = (size_t)widthInit * heightInit;
        void *d_stack = nullptr, *d_out = nullptr;
        float **fin = alloc_planes(3, n);
        int st = ugsm_dev_alloc(ctx_, &d_stack, (long long)(3 * sn * sizeof(float)));
        if (st == UGSM_OK) st = ugsm_dev_alloc(ctx_, &d_out, (long long)(3 * n * sizeof(float)));
        for (int c = 0; c < 3 && st == UGSM_OK; c++)
            for (int k = 0; k < F && st == UGSM_OK; k++)
                st = ugsm_copy_to_device(ctx_, (float *)d_stack + c * sn + k * fn, foveated[k][c], (long long)(fn * sizeof(float)));
        if (st == UGSM_OK)
            st = ugsm_reconstruct_full(ctx_, 0, (float *)d_stack, (float *)d_stack + sn, (float *)d_stack + 2 * sn, widthInit, heightInit, 0, 0,
                                       (float *)d_out);
        if (st == UGSM_OK) st = ugsm_wait(ctx_, 0);
        for (int c = 0; c < 3 && st == UGSM_OK; c++) st = ugsm_copy_to_host(ctx_, fin[c], (float *)d_out + c * n, (long long)(n * sizeof(float)));
        if (d_stack) ugsm_dev_free(ctx_, d_stack);
        if (d_out) ugsm_dev_free(ctx_, d_out);
        if (st != UGSM_OK) return fail(fin, 3, st);
        return fin;
    }

    // MatchGPULib.cpp:1445-1518.  right[j] = imageW*imageH floats for j < channels, disparity[0] / disparity[1] the horizontal / vertical
    // field.  Returns `channels` malloc'd planes: right[j] fetched where the matcher fetches it under the field (include/ugsm.h, "the warp").
    float **warpRightImage(float **right, float **disparity, int channels, int imageW, int imageH)
    {
        if (!right || !disparity || channels < 1 || imageW < 1 || imageH < 1) return nullptr;
        const size_t n = (size_t)imageW * imageH;
        void *d_src = nullptr, *d_disp = nullptr, *d_dst = nullptr;
        float **out = alloc_planes(channels, n);
        int st = ugsm_dev_alloc(ctx_, &d_src, (long long)(channels * n * sizeof(float)));
        if (st == UGSM_OK) st = ugsm_dev_alloc(ctx_, &d_disp, (long long)(2 * n * sizeof(float)));
        if (st == UGSM_OK) st = ugsm_dev_alloc(ctx_, &d_dst, (long long)(channels * n * sizeof(float)));
        for (int j = 0; j < channels && st == UGSM_OK; j++) st = ugsm_copy_to_device(ctx_, (float *)d_src + j * n, right[j], (long long)(n * sizeof(float)));
        for (int k = 0; k < 2 && st == UGSM_OK; k++) st = ugsm_copy_to_device(ctx_, (float *)d_disp + k * n, disparity[k], (long long)(n * sizeof(float)));
        if (st == UGSM_OK) st = ugsm_warp_planes(ctx_, 0, (float *)d_src, channels, imageW, imageH, (float *)d_disp, (float *)d_disp + n, (float *)d_dst);
        if (st == UGSM_OK) st = ugsm_wait(ctx_, 0);
        for (int j = 0; j < channels && st == UGSM_OK; j++) st = ugsm_copy_to_host(ctx_, out[j], (float *)d_dst + j * n, (long long)(n * sizeof(float)));
        for (void *p : {d_src, d_disp, d_dst})
            if (p) ugsm_dev_free(ctx_, p);
        if (st != UGSM_OK) return fail(out, channels, st);
        return out;
    }

    // (not in the reference's library: its point-cloud node fills range_map on the host, getPointCloud.cpp:730-758)  match(L, R, 0) and its
    // REP 118 depth image registered to the left camera (ugsm_match_full_depth): p->format UGSM_DEPTH_32F -- float metres, NaN for no reading --
    // or UGSM_DEPTH_16U -- uint16 millimetres, 0 for no reading; P1, P2 the 3x4 projection matrices, row-major.  Returns the image, malloc'd:
    // *dw x *dh elements, row-major, the payload of a sensor_msgs::Image with step = *dw * size.  finDisp (may be null): where given, the match's
    // planes come down too, as match returns them; otherwise only the image crosses the bus.
    template <class ImgPtr>
    void *depthImage(ImgPtr L, ImgPtr R, const double *P1, const double *P2, const ugsm_depth_params *p, int *dw, int *dh, float ***finDisp = nullptr)
    {
        if (finDisp) *finDisp = nullptr;
        foveatedmatching = 0;
        const int W = L->image.cols, H = L->image.rows;
        if (!p || !dw || !dh || R->image.cols != W || R->image.rows != H || ugsm_depth_image_size(W, H, p->factor, dw, dh) != UGSM_OK) return nullptr;
        void *img = std::malloc((size_t)*dw * *dh * (p->format == UGSM_DEPTH_16U ? 2 : 4));
        float **fin = finDisp ? alloc_planes(3, (size_t)W * H) : nullptr;
        const int st = img ? ugsm_match_full_depth(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, P1, P2, p, img, fin ? fin[0] : nullptr,
                                                   fin ? fin[1] : nullptr, fin ? fin[2] : nullptr)
                           : UGSM_ERR_NOMEM;
        if (st != UGSM_OK) {
            std::free(img);
            if (fin) fail(fin, 3, st);
            else report(st);
            return nullptr;
        }
        if (finDisp) *finDisp = fin;
        return img;
    }
    // ... and of a fovea stack as matchStack returns it (foveated[k][c] = fovW*fovH floats, c = 0, 1, 2: dx, dy, conf) for a rows x cols frame:
    // every level's image in one launch (ugsm_depth_image_fovea, UGSM_DEPTH_ALL_LEVELS), laid out level after level, level 0 first --
    // foveatelevel * *dh rows of *dw elements.  valid (may be null): foveatelevel counts of valid pixels.
    void *depthImageStack(float ***foveated, int cols, int rows, const double *P1, const double *P2, const ugsm_depth_params *p, int *dw, int *dh,
                          unsigned long long *valid = nullptr)
    {
        const int F = foveatelevel;
        int fw = 0, fh = 0;
        if (!foveated || !p || !dw || !dh || ugsm_fovea_dims(cols, rows, 14, F, &fw, &fh) != UGSM_OK ||
            ugsm_depth_image_size(fw, fh, p->factor, dw, dh) != UGSM_OK)
            return nullptr;
        const size_t fn = (size_t)fw * fh, sn = (size_t)F * fn, bytes = (size_t)F * *dw * *dh * (p->format == UGSM_DEPTH_16U ? 2 : 4);
        void *d_stack = nullptr, *d_img = nullptr, *d_valid = nullptr, *img = std::malloc(bytes);
        int st = img ? ugsm_dev_alloc(ctx_, &d_stack, (long long)(3 * sn * sizeof(float))) : UGSM_ERR_NOMEM;
        if (st == UGSM_OK) st = ugsm_dev_alloc(ctx_, &d_img, (long long)bytes);
        if (st == UGSM_OK) st = ugsm_dev_alloc(ctx_, &d_valid, (long long)(F * sizeof(unsigned long long)));
        for (int k = 0; k < F && st == UGSM_OK; k++)
            for (int c = 0; c < 3 && st == UGSM_OK; c++)
                st = ugsm_copy_to_device(ctx_, (float *)d_stack + c * sn + k * fn, foveated[k][c], (long long)(fn * sizeof(float)));
        if (st == UGSM_OK)
            st = ugsm_depth_image_fovea(ctx_, 0, (float *)d_stack, (float *)d_stack + sn, (float *)d_stack + 2 * sn, cols, rows, 0, 0, UGSM_DEPTH_ALL_LEVELS,
                                        P1, P2, p, d_img, (unsigned long long *)d_valid);
        if (st == UGSM_OK) st = ugsm_wait(ctx_, 0);
        if (st == UGSM_OK) st = ugsm_copy_to_host(ctx_, img, d_img, (long long)bytes);
        if (st == UGSM_OK && valid) st = ugsm_copy_to_host(ctx_, valid, d_valid, (long long)(F * sizeof(unsigned long long)));
        for (void *q : {d_stack, d_img, d_valid})
            if (q) ugsm_dev_free(ctx_, q);
        if (st != UGSM_OK) {
            std::free(img);
            report(st);
            return nullptr;
        }
        return img;
    }

    // ... and of the WHOLE frame from a foveated match (ugsm_match_foveated_depth): matchStack's match at window offset (off_x, off_y) and one
    // *dw x *dh image of the rows x cols frame from its stack -- what hierarchicalDisparity followed by the depth image of that field gives,
    // without the field.  Only the image crosses the bus.  (depthImageStack keeps its per-level meaning.)
    template <class ImgPtr>
    void *depthImageFrame(ImgPtr L, ImgPtr R, const double *P1, const double *P2, const ugsm_depth_params *p, int *dw, int *dh, int off_x = 0, int off_y = 0)
    {
        foveatedmatching = 1;
        const int W = L->image.cols, H = L->image.rows;
        if (!p || !dw || !dh || R->image.cols != W || R->image.rows != H || ugsm_depth_image_size(W, H, p->factor, dw, dh) != UGSM_OK) return nullptr;
        void *img = std::malloc((size_t)*dw * *dh * (p->format == UGSM_DEPTH_16U ? 2 : 4));
        const int st = img ? ugsm_match_foveated_depth(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, off_x, off_y, P1, P2, p, img, nullptr,
                                                       nullptr, nullptr)
                           : UGSM_ERR_NOMEM;
        if (st != UGSM_OK) {
            std::free(img);
            report(st);
            return nullptr;
        }
        return img;
    }

    // ---- the pipelined twin of match / matchStack / matchStackPyramid (not in the reference): include/ugsm.h, "the queue" ------------
    // The images are copied into page-locked staging memory of the library before the call returns (the cv_bridge image may be freed);
    // the result comes out of nextDone, in arrival order.  Every call flushes: a frame starts at once if a slot is free, and under load
    // the backlog batches itself.
    template <class ImgPtr>
    int enqueueMatch(ImgPtr L, ImgPtr R, uint64_t tag)
    {
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return UGSM_ERR_SIZE_MISMATCH;
        int st = ugsm_enqueue_full_managed(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, tag);
        if (st == UGSM_OK) { kinds_[tag] = Kind{false, false, W, H, false, false}; st = ugsm_flush(ctx_); }
        return report(st);
    }
    template <class ImgPtr>
    int enqueueStack(ImgPtr L, ImgPtr R, bool want_pyramids, uint64_t tag)
    {
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return UGSM_ERR_SIZE_MISMATCH;
        if (ugsm_fovea_dims(W, H, 14, foveatelevel, &fovW, &fovH) != UGSM_OK) return UGSM_ERR_BAD_ARG;
        int st = ugsm_enqueue_foveated_managed(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, 0, 0, want_pyramids ? 1 : 0, tag);
        if (st == UGSM_OK) { kinds_[tag] = Kind{true, want_pyramids, W, H, false, false}; st = ugsm_flush(ctx_); }
        return report(st);
    }
    // ... and with the pair's coloured cloud (include/ugsm.h, "the cloud from the queue"): the cloud of doReconstructionRGB /
    // doReconstructionRGB_FOV made on the device behind the match and lent through nextDone's Done::cloud.  spec: P1, P2, the cloud's
    // parameters, max_points, and want_planes -- 0: the result planes are not downloaded at all (Done::planes stay null).
    template <class ImgPtr>
    int enqueueMatchCloud(ImgPtr L, ImgPtr R, const ugsm_queue_cloud &spec, uint64_t tag)
    {
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return UGSM_ERR_SIZE_MISMATCH;
        int st = ugsm_enqueue_full_cloud_managed(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, &spec, tag);
        if (st == UGSM_OK) { kinds_[tag] = Kind{false, false, W, H, true, false}; st = ugsm_flush(ctx_); }
        return report(st);
    }
    template <class ImgPtr>
    int enqueueStackCloud(ImgPtr L, ImgPtr R, const ugsm_queue_cloud &spec, uint64_t tag)
    {
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return UGSM_ERR_SIZE_MISMATCH;
        if (ugsm_fovea_dims(W, H, 14, foveatelevel, &fovW, &fovH) != UGSM_OK) return UGSM_ERR_BAD_ARG;
        int st = ugsm_enqueue_foveated_cloud_managed(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, 0, 0, &spec, tag);
        if (st == UGSM_OK) { kinds_[tag] = Kind{true, false, W, H, true, false}; st = ugsm_flush(ctx_); }
        return report(st);
    }
    // ... and checked (include/ugsm.h, "checked pairs through the queue"): both directions of the pairs of a call in lockstep with THIS pair's
    // tau (> 0), whatever setLRCheck holds; the planes nextDone lends are the checked forward field.  want_back: the right camera's checked
    // planes too, through Done::checked.back.  Full mode only (the foveated queue forms are checked through setLRCheck's UGSM_LR_FOVEATED).
    template <class ImgPtr>
    int enqueueMatchChecked(ImgPtr L, ImgPtr R, float tau, bool want_back, uint64_t tag)
    {
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return UGSM_ERR_SIZE_MISMATCH;
        int st = ugsm_enqueue_full_checked_managed(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, tau, want_back ? 1 : 0, tag);
        if (st == UGSM_OK) { kinds_[tag] = Kind{false, false, W, H, false, true}; st = ugsm_flush(ctx_); }
        return report(st);
    }
    template <class ImgPtr>
    int enqueueMatchCheckedCloud(ImgPtr L, ImgPtr R, float tau, bool want_back, const ugsm_queue_cloud &spec, uint64_t tag)
    {
        const int W = L->image.cols, H = L->image.rows;
        if (R->image.cols != W || R->image.rows != H) return UGSM_ERR_SIZE_MISMATCH;
        int st = ugsm_enqueue_full_checked_cloud_managed(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, tau, want_back ? 1 : 0, &spec, tag);
        if (st == UGSM_OK) { kinds_[tag] = Kind{false, false, W, H, true, true}; st = ugsm_flush(ctx_); }
        return report(st);
    }
    int outstanding() const { return (int)kinds_.size(); }
    // What nextDone hands out.  planes: full mode dispH, dispV, dispC (rows x cols); foveated stackH, stackV, stackC ((levels fovH) x fovW,
    // finest level first -- the layout the node publishes, UG_GPU_matcher.cpp:293-320) and, if asked for, the L / R pyramid stacks
    // ((levels 3 fovH) x fovW, :203-226).  The planes belong to the library and stay valid until the next nextDone.
    struct Done {
        uint64_t tag;
        int status;      // UGSM_OK, or the status of the library call the pair went out in (planes are then null: nothing to publish)
        bool foveated, pyramids;
        int rows, cols;  // of the image
        float *planes[5];
        bool has_cloud;           // the pair was enqueued with enqueueMatchCloud / enqueueStackCloud and its call succeeded: ...
        ugsm_cloud_result cloud;  // ... its cloud (ugsm_done_cloud): page-locked records of the library, valid until the next nextDone
        bool is_checked;              // the pair was enqueued with enqueueMatchChecked[Cloud] and its call succeeded: ...
        ugsm_checked_result checked;  // ... the pixels its check marked and, with want_back, the right camera's planes (ugsm_done_checked)
    };
    // true: *out filled -- the oldest pair has been REPORTED and no longer counts as outstanding; out->status says how its call went (a
    // failed call: logged to stderr, planes null; the caller drops whatever it keeps under the tag).  false: nothing outstanding, or
    // (block == false) the oldest pair has not finished.
    bool nextDone(bool block, Done *out)
    {
        ugsm_completion c;
        const int st = ugsm_next_done(ctx_, &c, block ? 1 : 0);
        if (st != UGSM_OK) { if (st != UGSM_PENDING && st != UGSM_EMPTY) report(st); return false; }
        const Kind k = kinds_[c.tag];
        kinds_.erase(c.tag);
        out->tag = c.tag; out->status = report(c.status); out->foveated = k.foveated; out->pyramids = k.pyramids; out->rows = k.H; out->cols = k.W;
        for (int i = 0; i < 5; i++) out->planes[i] = c.status == UGSM_OK ? c.result[i] : nullptr;
        out->cloud = ugsm_cloud_result();
        out->has_cloud = k.cloud && c.status == UGSM_OK && report(ugsm_done_cloud(ctx_, &out->cloud)) == UGSM_OK;
        out->checked = ugsm_checked_result();
        out->is_checked = k.checked && c.status == UGSM_OK && report(ugsm_done_checked(ctx_, &out->checked)) == UGSM_OK;
        return true;
    }

private:
    ugsm_ctx *ctx_;
    int levels_ = 0;  // the context's pyramid levels (matchCoarse / matchFine size a level's field by them)
    struct Kind { bool foveated, pyramids; int W, H; bool cloud, checked; };
    std::map<uint64_t, Kind> kinds_;
    int report(int st)
    {
        if (st != UGSM_OK) std::fprintf(stderr, "ugsm: %s: %s\n", ugsm_status_string(st), ugsm_last_error(ctx_));
        return st;
    }

    static float **alloc_planes(int n, size_t px)
    {
        float **p = (float **)std::malloc(n * sizeof(float *));
        for (int i = 0; i < n; i++) p[i] = (float *)std::malloc(px * sizeof(float));
        return p;
    }
    float **fail(float **p, int n, int st)
    {
        std::fprintf(stderr, "ugsm: %s: %s\n", ugsm_status_string(st), ugsm_last_error(ctx_));
        for (int i = 0; i < n; i++) std::free(p[i]);
        std::free(p);
        return nullptr;
    }
    template <class ImgPtr>
    float ***stack(ImgPtr L, ImgPtr R, float ***leftFov, float ***rightFov)
    {
        const int W = L->image.cols, H = L->image.rows, F = foveatelevel;
        if (R->image.cols != W || R->image.rows != H) return nullptr;
        if (ugsm_fovea_dims(W, H, 14, F, &fovW, &fovH) != UGSM_OK) return nullptr;
        const size_t fn = (size_t)fovW * fovH, sn = fn * F;
        float *sh = (float *)std::malloc(3 * sn * sizeof(float));
        float *pl = leftFov ? (float *)std::malloc(3 * sn * sizeof(float)) : nullptr;
        float *pr = rightFov ? (float *)std::malloc(3 * sn * sizeof(float)) : nullptr;
        const int st = ugsm_match_foveated(ctx_, L->image.data, R->image.data, W, H, (int)L->image.step, 0, 0, sh, sh + sn,
                                           sh + 2 * sn, pl, pr);
        float ***disp = nullptr;
        if (st == UGSM_OK) {
            disp = (float ***)std::malloc(F * sizeof(float **));
            for (int k = 0; k < F; k++) {
                disp[k] = alloc_planes(3, fn);
                for (int c = 0; c < 3; c++) std::memcpy(disp[k][c], sh + c * sn + k * fn, fn * sizeof(float));
                for (int c = 0; c < 3 && pl; c++) std::memcpy(leftFov[k][c], pl + ((size_t)k * 3 + c) * fn, fn * sizeof(float));
                for (int c = 0; c < 3 && pr; c++) std::memcpy(rightFov[k][c], pr + ((size_t)k * 3 + c) * fn, fn * sizeof(float));
            }
        } else {
            std::fprintf(stderr, "ugsm: %s: %s\n", ugsm_status_string(st), ugsm_last_error(ctx_));
        }
        std::free(sh);
        std::free(pl);
        std::free(pr);
        return disp;
    }
};
