// ugsm_cloud.cpp -- row f-1 of the runtime: triangulation and the coloured point clouds (getPointCloud.cpp), on the slots of ugsm_runtime.cpp.
// The fovea forms' geometry and the coverage rule of the merged clouds (host only), the slot-level entry points behind one description of a
// cloud call (cloud_call_args) and one preamble (cloud_begin), and the queue's cloud calls (CtxHooks::cloud_submit / cloud_finish), which use
// both.  Every cloud kernel is cloud_tile (ugsm_kernels_cloud.hip); the planes and the depth images are k_triangulate[_fovea]'s (ugsm_kernels_depth.hip).
#include "ugsm_slot.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>

using namespace ugsm;

// What the depth calls refuse about their parameters and the planes' size (no device needed), and the image's size.  have_conf: the call has
// a confidence plane.
int ugsm::depth_params_ok(const ugsm_depth_params *p, bool have_conf, int pw, int ph, int *dw, int *dh)
{
    if (!p || pw < 1 || ph < 1 || (long long)pw * ph > kMaxPixels) return UGSM_ERR_BAD_ARG;
    if (p->format != UGSM_DEPTH_32F && p->format != UGSM_DEPTH_16U) return UGSM_ERR_BAD_ARG;
    if (!(std::isfinite(p->unit) && p->unit > 0.0f)) return UGSM_ERR_BAD_ARG;
    if (!keep_window_ok(p->min_conf, p->z_min, p->z_max, have_conf)) return UGSM_ERR_BAD_ARG;
    return ugsm_depth_image_size(pw, ph, p->factor, dw, dh);
}

namespace {

// the sampled grid along one side: the pixels 0, s, 2 s, ... below n
int sampled(int n, int s) { return (n + s - 1) / s; }

// The resized map of pw x ph planes: cv::Size(pw * f, ph * f) -- float products, truncated -- and cv::resize's scales (resize.cpp: inv_scale =
// (double)dsize / ssize, scale = 1. / inv_scale).  dw = 0: no such map -- a factor outside (0, 1], or one that leaves a side at 0.
struct ResizedGrid {
    int dw = 0, dh = 0;
    CloudResize rz{};
};
ResizedGrid resized_grid(int pw, int ph, float factor, int colour_mapped = 0)
{
    ResizedGrid g;
    if (pw < 1 || ph < 1 || !(factor > 0.0f && factor <= 1.0f)) return g;
    const int dw = (int)((float)pw * factor), dh = (int)((float)ph * factor);
    if (dw < 1 || dh < 1) return g;
    g.dw = dw;
    g.dh = dh;
    g.rz.scale_x = 1. / ((double)dw / pw);
    g.rz.scale_y = 1. / ((double)dh / ph);
    g.rz.factor = factor;
    g.rz.same_size = dw == pw && dh == ph;
    g.rz.colour_mapped = colour_mapped;
    return g;
}

// one launch (or a count launch and the cloud's) in the statistics' bracket, and what it reports
template <class F>
int timed_launch(ugsm_ctx *ctx, Slot *s, int slot, double points, F &&launch)
{
    {
        Timer t(ctx, s, slot, KC_MISC, points);
        launch();
    }
    HIPCHK(ctx, hipGetLastError());
    return UGSM_OK;
}

// ugsm_fovea_level_mapping for every level of the stack: the reference's centred margins for any fovea_levels (its `scaled` is
// F-1-k), moved by this build's window offset -- level k's clamped offset ex[k] (fovea_geometry), in level-0 pixels
int fovea_level_mappings(int W, int H, int levels, int F, int off_x, int off_y, int *fw, int *fh, int *left, int *upper, float *scale)
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    if (F < 2 || F > levels || levels > UGSM_MAX_LEVELS) return UGSM_ERR_BAD_ARG;
    UCHK(level_dims(W, H, F, w, h));  // (only the stack's F levels enter: a cloud of a given stack does not ask whether the coarse levels below it exist)
    FoveaGeom g;
    fovea_geometry(w, h, F, off_x, off_y, g);
    *fw = g.fw;
    *fh = g.fh;
    for (int k = 0; k < F; k++) {
        const int ex = k < F - 1 ? g.ox[k] - (w[k] / 2 - g.fw / 2) : 0, ey = k < F - 1 ? g.oy[k] - (h[k] / 2 - g.fh / 2) : 0;
        left[k] = w[0] / 2 - w[F - 1 - k] / 2 + (int)lrint(ex * pow(kScale, k));
        upper[k] = h[0] / 2 - h[F - 1 - k] / 2 + (int)lrint(ey * pow(kScale, k));
        scale[k] = powf((float)1.41421356237309504880, (float)k);  // as ugsm_fovea_mapping for destination level 0
    }
    return UGSM_OK;
}

// The coverage rule along one axis (include/ugsm.h): pixel i of level k, at x1 = (float)m + (float)i * sc, is covered when
// x1 >= (float)m_fine && x1 + sc <= (float)m_fine + (float)n * sc_fine, every operation in binary32.  Monotone in i, so the covered
// pixels are one interval [i0, i1); of the sampled grid (pixel = index * s) that is [c0, c1).  x1 never falls as i grows (i is exact in
// binary32, and a rounded product and a rounded sum keep the order of their operands), so the first test turns true once and the second
// false once: two bisections, the same interval a scan over the pixels finds (the merged cloud of several windows asks for up to 31
// rectangles for each of up to 97 entries per call).
void covered_interval(int n, int m, float sc, int m_fine, float sc_fine, int s, int *c0, int *c1)
{
    const float lo = (float)m_fine, hi = (float)m_fine + (float)n * sc_fine;
    auto first = [&](int from, auto test) {  // the first i in [from, n) that passes a test which stays passed; n: none
        int a = from, b = n;
        while (a < b) {
            const int mid = a + (b - a) / 2;
            if (test((float)m + (float)mid * sc)) b = mid;
            else a = mid + 1;
        }
        return a;
    };
    int i0 = first(0, [&](float x1) { return x1 >= lo; });
    int i1 = first(i0, [&](float x1) { return !(x1 + sc <= hi); });
    if (i1 <= i0) i0 = i1 = n;  // (nothing covered)
    *c0 = (i0 + s - 1) / s;
    *c1 = (i1 + s - 1) / s;
    if (*c1 < *c0) *c1 = *c0;
}

// ---- the merged cloud of several windows of one pair (ugsm_point_cloud_fovea_multi; the rule across windows: include/ugsm.h) ----------
struct MultiCloud {
    int n, F, E, fw, fh, wc, hc, s;
    int left[UGSM_MAX_BATCH][UGSM_MAX_LEVELS], upper[UGSM_MAX_BATCH][UGSM_MAX_LEVELS];
    float scale[UGSM_MAX_LEVELS];
};

int cloud_multi_geometry(int W, int H, int levels, int F, int n, const int *off_x, const int *off_y, int sampling, MultiCloud &g)
{
    if (n < 1 || n > UGSM_MAX_BATCH || sampling < 1) return UGSM_ERR_BAD_ARG;
    for (int j = 0; j < n; j++)
        UCHK(fovea_level_mappings(W, H, levels, F, off_x ? off_x[j] : 0, off_y ? off_y[j] : 0, &g.fw, &g.fh, g.left[j], g.upper[j], g.scale));
    g.n = n;
    g.F = F;
    g.E = (F - 1) * n + 1;
    g.s = sampling;
    g.wc = sampled(g.fw, sampling);
    g.hc = sampled(g.fh, sampling);
    return UGSM_OK;
}

// Entry e's row of the kernel's table, its planes apart: the mapping, the rectangles the entry leaves out -- (a) inside level k-1 of any
// window, (b) inside level k of a higher-numbered window; each a column interval times a row interval (covered_interval) -- the column
// segments between the rectangles' edges, and the entry's dense records.  `first`: the records of the entries before it.
void cloud_multi_entry(const MultiCloud &g, int e, long long first, CloudEntry &en)
{
    const int k = e / g.n, j = e - k * g.n;  // (the last entry: level F-1 of window 0)
    en = CloudEntry{};
    en.left_margin = g.left[j][k];
    en.upper_margin = g.upper[j][k];
    en.scale = g.scale[k];
    auto add = [&](int i, int m) {
        CloudRect q;
        covered_interval(g.fw, g.left[j][k], g.scale[k], g.left[i][m], g.scale[m], g.s, &q.cx0, &q.cx1);
        covered_interval(g.fh, g.upper[j][k], g.scale[k], g.upper[i][m], g.scale[m], g.s, &q.cy0, &q.cy1);
        if (q.cx0 < q.cx1 && q.cy0 < q.cy1 && en.nrect < kCloudMaxRects) en.rect[en.nrect++] = q;
    };
    if (k >= 1)
        for (int i = 0; i < g.n; i++) add(i, k - 1);
    if (k <= g.F - 2)
        for (int i = j + 1; i < g.n; i++) add(i, k);
    // the segments: between two neighbouring edges the same rectangles hold every column, so every column keeps the same number of rows
    int xs[kCloudMaxSegs + 1], nx = 0;
    xs[nx++] = 0;
    for (int i = 0; i < en.nrect; i++)
        for (int x : {en.rect[i].cx0, en.rect[i].cx1})
            if (x > 0 && x < g.wc) xs[nx++] = x;
    std::sort(xs, xs + nx);
    nx = (int)(std::unique(xs, xs + nx) - xs);
    long long records = 0;
    for (int sg = 0; sg < nx; sg++) {
        std::pair<int, int> rows[kCloudMaxRects];
        int nr = 0;
        for (int i = 0; i < en.nrect; i++)
            if (en.rect[i].cx0 <= xs[sg] && xs[sg] < en.rect[i].cx1) rows[nr++] = {en.rect[i].cy0, en.rect[i].cy1};
        std::sort(rows, rows + nr);
        int out = 0, reach = 0;  // the length of the union of the row intervals
        for (int i = 0; i < nr; i++) {
            out += std::max(rows[i].second - std::max(rows[i].first, reach), 0);
            reach = std::max(reach, rows[i].second);
        }
        en.seg_x[sg] = xs[sg];
        en.seg_rows[sg] = g.hc - out;
        en.seg_first[sg] = (unsigned)records;
        records += (long long)((sg + 1 < nx ? xs[sg + 1] : g.wc) - xs[sg]) * (g.hc - out);
    }
    en.nseg = nx;
    en.first = first;
    en.points = records;
}

// The table of the whole stack's cloud (ugsm_point_cloud_fovea_all): each level's planes, mapping, covered rectangle and dense records.  It is
// the merged cloud of ONE window: entry k is level k, and what it leaves out is at most one rectangle -- the part inside level k-1.
int cloud_stack_table(int W, int H, int levels, int F, int off_x, int off_y, int sampling, CloudStack &sk, int *fw_out, int *fh_out)
{
    MultiCloud g;
    UCHK(cloud_multi_geometry(W, H, levels, F, 1, &off_x, &off_y, sampling, g));
    sk = CloudStack{};
    sk.F = F;
    sk.strips = cloud_strips(g.wc);
    long long first = 0;
    for (int k = 0; k < F; k++) {
        CloudEntry en;
        cloud_multi_entry(g, k, first, en);
        CloudLevel &lv = sk.lv[k];
        lv.plane = (long long)k * g.fw * g.fh;
        lv.left_margin = en.left_margin;
        lv.upper_margin = en.upper_margin;
        lv.scale = en.scale;
        const CloudRect out = en.nrect ? en.rect[0] : CloudRect{};
        lv.cx0 = out.cx0;
        lv.cx1 = out.cx1;
        lv.cy0 = out.cy0;
        lv.cy1 = out.cy1;
        lv.first = first;
        lv.points = en.points;
        first += en.points;
    }
    if (fw_out) *fw_out = g.fw;
    if (fh_out) *fh_out = g.fh;
    return UGSM_OK;
}

// A cloud call, described: what the points come from, the image that colours them, where they go.
struct CloudFrom {
    const float *dx, *dy, *conf;  // pw x ph planes, or (fovea) the stacks those are level `level` of; conf may be null
    int pw, ph;
    bool fovea = false;           // the fovea forms: the stack level, and its mapping (ugsm_fovea_mapping)
    int level = 0, left_margin = 0, upper_margin = 0;
    float scale = 0.0f;
};
struct CloudImage {
    const uint8_t *rgb;
    int W, H, stride;
};
struct CloudTo {
    void *points;
    long long cap;
    long long *count;
};

// The checks every cloud call shares (no device needed), in the one order they have always had, then the call's CloudArgs (conf is only
// read by a compact cloud).  resized (the resized forms, which take no sampling: p->sampling 1): the map, whose grid the arguments get.
int cloud_call_args(const ugsm_ctx *ctx, const CloudFrom &from, const CloudImage &im, const double *P1, const double *P2, const ugsm_cloud_params *p,
                    const CloudTo &to, CloudArgs &a, const ResizedGrid *resized = nullptr)
{
    if (!ctx || !from.dx || !from.dy || !im.rgb || !P1 || !P2 || !p || !to.points || !to.count) return UGSM_ERR_BAD_ARG;
    if (im.W < 1 || im.H < 1 || from.pw < 1 || from.ph < 1 || (long long)im.W * im.H > kMaxPixels || (long long)from.pw * from.ph > kMaxPixels)
        return UGSM_ERR_BAD_ARG;
    if (input_status(ctx, im.W, im.stride, im.rgb) != UGSM_OK || !cloud_records_ok(*p)) return UGSM_ERR_BAD_ARG;
    if (!keep_window_ok(p->min_conf, p->z_min, p->z_max, from.conf != nullptr)) return UGSM_ERR_BAD_ARG;
    if (to.cap < 0 || ((uintptr_t)to.points & 15) || ((uintptr_t)to.count & 7)) return UGSM_ERR_BAD_ARG;
    if (resized && (p->sampling != 1 || resized->dw < 1)) return UGSM_ERR_BAD_ARG;
    if (from.fovea && (from.level < 0 || from.level >= UGSM_MAX_LEVELS || !std::isfinite(from.scale))) return UGSM_ERR_BAD_ARG;
    const size_t lvl = from.fovea ? (size_t)from.level * from.pw * from.ph : 0;
    a = CloudArgs{};
    a.dx = from.dx + lvl;
    a.dy = from.dy + lvl;
    a.conf = p->compact && from.conf ? from.conf + lvl : nullptr;
    a.pw = from.pw;
    a.ph = from.ph;
    a.rgb = im.rgb;
    a.W = im.W;
    a.H = im.H;
    a.stride = im.stride;
    a.s = p->sampling;
    a.format = p->format;
    a.compact = p->compact != 0;
    a.min_conf = p->min_conf;
    a.z_min = p->z_min;
    a.z_max = p->z_max;
    a.left_margin = from.left_margin;
    a.upper_margin = from.upper_margin;
    a.scale = from.scale;
    a.points = to.points;
    a.cap = to.cap;
    a.count = to.count;
    if (resized) {
        a.wc = resized->dw;
        a.hc = resized->dh;
    }
    return UGSM_OK;
}
// The words of a compact cloud's count buffer (CloudArgs.cnt) over `entries` virtual grids of wc columns -- the levels of a stack, the entries
// of a merged cloud: the entries' (column, chunk) counts, then their column totals and strip totals.
size_t cloud_cnt_words(int entries, int wc, int nchunk) { return (size_t)entries * ((size_t)wc * nchunk + wc + cloud_strips(wc)); }

// What every cloud derives before its launch and no slot is needed for: the sampled grid (unless the resized forms have theirs), its chunks, the
// input format, and the region a compact cloud of `entries` virtual grids takes of a count buffer -- its (column, chunk) counts, then the
// totals, which are zeroed before the launch.
struct CloudRegion {
    size_t counts, words;
};
CloudRegion cloud_grid(const ugsm_ctx *ctx, CloudArgs &a, int entries)
{
    if (!a.wc) {
        a.wc = sampled(a.pw, a.s);
        a.hc = sampled(a.ph, a.s);
    }
    a.nchunk = cloud_chunks(a.hc);
    a.fmt = ctx->hooks.input_format;
    a.cnt = nullptr;
    return {(size_t)entries * a.wc * a.nchunk, cloud_cnt_words(entries, a.wc, a.nchunk)};
}

// What every slot-level cloud does before its launch: it takes the slot and sets the device, derives the grid (cloud_grid) and, for a compact
// cloud, makes the slot's count buffer hold the region and zeroes its totals on the slot's stream.  table (the merged cloud of several
// windows): before that, the call's turn of the slot's upload ring -- one row per entry, for the caller to fill and upload.
int cloud_begin(ugsm_ctx *ctx, int slot, CloudArgs &a, int entries, Slot **out, CloudEntry **table = nullptr)
{
    UCHK(get_slot(ctx, slot, out));
    Slot &s = **out;
    SlotCloud &c = s.cloud;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    const CloudRegion r = cloud_grid(ctx, a, entries);
    if (table) UCHK(c.mc.begin(ctx, s.st, (size_t)entries, table));
    if (!a.compact) return UGSM_OK;
    if (r.words > c.cnt.cap) HIPCHK(ctx, hipStreamSynchronize(s.st));  // (the buffer being replaced may still be read by an earlier cloud)
    UCHK(c.cnt.grow(ctx, r.words));
    a.cnt = c.cnt;
    HIPCHK(ctx, hipMemsetAsync(a.cnt + r.counts, 0, (r.words - r.counts) * sizeof(unsigned), s.st));  // (the totals)
    return UGSM_OK;
}

int point_cloud(ugsm_ctx *ctx, int slot, CloudArgs &a, bool fovea, const double *P1, const double *P2, const CloudResize *rz = nullptr)
{
    Slot *s;
    UCHK(cloud_begin(ctx, slot, a, 1, &s));
    return timed_launch(ctx, s, slot, (double)a.wc * a.hc, [&] { launch_point_cloud(s->st, a, fovea, P1, P2, rz, ctx_lens(ctx)); });
}

// The depth image's checks (no device needed) and its kernel arguments.  dx, dy, conf: `in_levels` levels of pw x ph floats each (a field: 1;
// the fovea stacks: F); the call writes `levels` images of dw x dh elements behind each other and as many counts.
// in_floats (the whole-frame forms, whose inputs are not the image's size): the floats behind each of dx, dy, conf, else in_levels * pw * ph.
int depth_args_ok(const ugsm_ctx *ctx, const float *dx, const float *dy, const float *conf, int in_levels, int pw, int ph, int levels, const double *P1,
                  const double *P2, const ugsm_depth_params *p, const void *depth, const void *valid, DepthArgs &d, size_t in_floats = 0)
{
    if (!ctx || !dx || !dy || !P1 || !P2 || !depth) return UGSM_ERR_BAD_ARG;
    int dw, dh;
    UCHK(depth_params_ok(p, conf != nullptr, pw, ph, &dw, &dh));
    const size_t size = p->format == UGSM_DEPTH_16U ? 2 : 4;
    if (((uintptr_t)depth & (size - 1)) || ((uintptr_t)valid & 7)) return UGSM_ERR_BAD_ARG;
    if (((uintptr_t)dx | (uintptr_t)dy | (uintptr_t)conf) & 3) return UGSM_ERR_BAD_ARG;
    const uintptr_t o0 = (uintptr_t)depth, o1 = o0 + (size_t)levels * dw * dh * size, in_bytes = (in_floats ? in_floats : (size_t)in_levels * pw * ph) * sizeof(float);
    for (const float *q : {dx, dy, conf})
        if (q && o0 < (uintptr_t)q + in_bytes && (uintptr_t)q < o1) return UGSM_ERR_BAD_ARG;  // (the image would overwrite what it is made from)
    d = DepthArgs{};
    d.conf = conf;
    d.out = const_cast<void *>(depth);
    d.valid = static_cast<unsigned long long *>(const_cast<void *>(valid));
    d.unit = p->unit;
    d.min_conf = p->min_conf;
    d.z_min = p->z_min;
    d.z_max = p->z_max;
    d.dw = dw;
    d.dh = dh;
    d.rz = resized_grid(pw, ph, p->factor).rz;
    return UGSM_OK;
}

// the slot, the device, the counts zeroed on the slot's stream, the launch (one for all `levels` images) in the statistics' misc class
template <class F>
int depth_image(ugsm_ctx *ctx, int slot, const DepthArgs &d, int levels, F &&launch)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (d.valid) HIPCHK(ctx, hipMemsetAsync(d.valid, 0, (size_t)levels * sizeof(unsigned long long), s->st));
    return timed_launch(ctx, s, slot, (double)levels * d.dw * d.dh, [&] { launch(s->st); });
}

// ---- the depth image of the whole frame from a fovea stack (ugsm_depth_image_fovea_full / _multi) ------------------------------------------
// The call's table goes up on the turns of the slot's one upload ring (SlotCloud::mc, the merged cloud's): its rows are raw memory to this
// call, as many CloudEntry rows as hold the n windows.
static_assert(alignof(CloudEntry) >= alignof(FrameWindow) && std::is_trivially_copyable<FrameWindow>::value, "FrameWindow rows in the ring's rows");
size_t frame_table_rows(int n) { return ((size_t)n * sizeof(FrameWindow) + sizeof(CloudEntry) - 1) / sizeof(CloudEntry); }

// What both forms derive and refuse before any device work: the levels' sizes and the n windows' origins (fovea_geometry, as
// ugsm_reconstruct_full[_multi] place them), the depth image's own checks on the W x H frame against stack 0's planes (depth_args_ok; sx, sy,
// sc: F x fh x fw floats each), and every further stack's overlap with the image.  stack: null (one window, the three planes apart), or the n
// stacks of three planes each.
int depth_frame_args(const ugsm_ctx *ctx, int n, const float *const *stack, const float *sx, const float *sy, const float *sc, int W, int H,
                     const int *off_x, const int *off_y, const double *P1, const double *P2, const ugsm_depth_params *p, const void *depth,
                     const void *valid, DepthArgs &d, DepthFrame &fr, FrameWindow *win)
{
    if (!ctx || n < 1 || n > UGSM_MAX_BATCH || W < 1 || H < 1 || (long long)W * H > kMaxPixels) return UGSM_ERR_BAD_ARG;
    const int levels = ctx->cfg.levels, F = ctx->cfg.fovea_levels;
    if (F < 2 || F > levels || levels > UGSM_MAX_LEVELS) return UGSM_ERR_BAD_ARG;
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, levels, w, h));  // (as ugsm_reconstruct_full: the context's whole pyramid must exist at this size)
    fr = DepthFrame{};
    fr.n = n;
    fr.F = F;
    for (int l = 0; l < F; l++) {
        fr.w[l] = w[l];
        fr.h[l] = h[l];
    }
    for (int j = 0; j < n; j++) {
        FoveaGeom g;
        fovea_geometry(w, h, F, off_x ? off_x[j] : 0, off_y ? off_y[j] : 0, g);
        fr.fw = g.fw;
        fr.fh = g.fh;
        win[j] = FrameWindow{};
        for (int l = 0; l < F - 1; l++) {
            win[j].ox[l] = g.ox[l];
            win[j].oy[l] = g.oy[l];
        }
        if (stack) {
            if (!stack[j]) return UGSM_ERR_BAD_ARG;
            win[j].stack = byte_diff(stack[j], stack[0]);
        }
    }
    const size_t plane = (size_t)F * fr.fw * fr.fh;
    if (stack) {
        sx = stack[0];
        sy = sx + plane;
        sc = sx + 2 * plane;
    }
    UCHK(depth_args_ok(ctx, sx, sy, sc, 1, W, H, 1, P1, P2, p, depth, valid, d, plane));
    const size_t image = (size_t)d.dw * d.dh * (p->format == UGSM_DEPTH_16U ? 2 : 4);
    for (int j = 1; stack && j < n; j++) {
        if ((uintptr_t)stack[j] & 3) return UGSM_ERR_BAD_ARG;
        if (overlap(depth, image, stack[j], 3 * plane * sizeof(float))) return UGSM_ERR_BAD_ARG;
    }
    return UGSM_OK;
}

// the slot, the table of n > 1 windows up on the slot's stream (nothing waits for the stream unless the ring has to grow), the count zeroed, the one launch
int depth_frame(ugsm_ctx *ctx, int slot, const float *sx, const float *sy, const double *P1, const double *P2, const DepthArgs &d, DepthFrame &fr,
                const FrameWindow *win, bool u16)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    if (fr.n > 1) {
        CloudEntry *rows;
        const size_t nrows = frame_table_rows(fr.n);
        UCHK(s->cloud.mc.begin(ctx, s->st, nrows, &rows));
        memcpy(static_cast<void *>(rows), win, (size_t)fr.n * sizeof(FrameWindow));
        UCHK(s->cloud.mc.upload(ctx, s->st, nrows));
        fr.table = reinterpret_cast<const FrameWindow *>(static_cast<const CloudEntry *>(s->cloud.mc.tab));
    }
    if (d.valid) HIPCHK(ctx, hipMemsetAsync(d.valid, 0, sizeof(unsigned long long), s->st));
    bool fits = true;
    UCHK(timed_launch(ctx, s, slot, (double)d.dw * d.dh,
                      [&] { fits = launch_depth_image_frame(s->st, sx, sy, P1, P2, d, fr, win, u16, ctx_lens(ctx)); }));
    return fits ? UGSM_OK : ctx_fail(ctx, UGSM_ERR_STATE, "a window of the stack leaves its level");
}

// A refusal of `call` names it in ugsm_last_error, in front of what the check itself had to say.
template <class F>
int named(ugsm_ctx *ctx, const char *call, F &&body)
{
    if (!ctx) return body();
    const std::string before = ctx->err;
    ctx->err.clear();
    const int st = body();
    if (st == UGSM_OK) ctx->err = before;
    else ctx->err = std::string(call) + ": " + (ctx->err.empty() ? ugsm_status_string(st) : ctx->err);
    return st;
}

constexpr size_t kCqWords = 1 + UGSM_MAX_LEVELS;  // a managed pair's count words: the count, the level counts

int queue_cloud_launch(ugsm_ctx *ctx, Slot &s, int si, int b0, int n, bool stack, const ugsm_queue_cloud *spec)
{
    const CloudPair &shape = s.cloud.cq_tab_h[b0];
    return timed_launch(ctx, &s, si, (double)n * (stack ? shape.sk.F : 1) * shape.a.wc * shape.a.hc,
                        [&] { launch_point_cloud_batch(s.st, s.cloud.cq_tab + b0, n, shape, stack, spec->P1, spec->P2); });
}

}  // namespace

extern "C" {

int ugsm_triangulate(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, int W, int H, const double *P1, const double *P2,
                     float *d_xyz)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_dispx || !d_dispy || !P1 || !P2 || !d_xyz || W < 1 || H < 1) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    return timed_launch(ctx, s, slot, (double)W * H, [&] { launch_triangulate(s->st, d_dispx, d_dispy, W, H, P1, P2, d_xyz, ctx_lens(ctx)); });
}

// CdynamicCalibration::left_marginOf_in / upper_marginOf_in / mapXcoord (getPointCloud.cpp:387-484)
int ugsm_fovea_mapping(int W, int H, int src_level, int dest_level, int *left_margin, int *upper_margin, float *scale)
{
    if (!left_margin || !upper_margin || !scale || W < 1 || H < 1) return UGSM_ERR_BAD_ARG;
    int scaled = 6 - src_level;  // :435 (the reference hard-codes its 7 fovea levels here)
    if (src_level < dest_level) scaled = src_level + dest_level;
    if (scaled < 0 || scaled >= 15 || dest_level < 0 || dest_level >= 15 || src_level < 0) return UGSM_ERR_BAD_ARG;
    int w[16], h[16];
    w[0] = W;
    h[0] = H;
    for (int i = 0; i < 14; i++) {  // :441-443
        w[i + 1] = (int)(w[i] / kScale);
        h[i + 1] = (int)(h[i] / kScale);
    }
    *left_margin = w[dest_level] / 2 - w[scaled] / 2;
    *upper_margin = h[dest_level] / 2 - h[scaled] / 2;
    const float root = (src_level < dest_level) ? (float)0.70710678118654752440 : (float)1.41421356237309504880;
    *scale = powf(root, (float)std::abs(src_level - dest_level));  // pow(float, float), :397
    return UGSM_OK;
}

long long ugsm_fovea_multi_cloud_points(int W, int H, int levels, int fovea_levels, int n, const int *off_x, const int *off_y, int sampling,
                                        long long *per_entry)
{
    MultiCloud g;
    if (cloud_multi_geometry(W, H, levels, fovea_levels, n, off_x, off_y, sampling, g) != UGSM_OK) return -1;
    long long total = 0;
    for (int e = 0; e < g.E; e++) {
        CloudEntry en;
        cloud_multi_entry(g, e, total, en);
        if (per_entry) per_entry[e] = en.points;
        total += en.points;
    }
    return total;
}

int ugsm_fovea_level_mapping(int W, int H, int levels, int fovea_levels, int off_x, int off_y, int src_level, int *left_margin,
                             int *upper_margin, float *scale)
{
    if (!left_margin || !upper_margin || !scale || src_level < 0 || src_level >= fovea_levels) return UGSM_ERR_BAD_ARG;
    int left[UGSM_MAX_LEVELS], upper[UGSM_MAX_LEVELS], fw, fh;
    float sc[UGSM_MAX_LEVELS];
    if (fovea_level_mappings(W, H, levels, fovea_levels, off_x, off_y, &fw, &fh, left, upper, sc) != UGSM_OK) return UGSM_ERR_BAD_ARG;
    *left_margin = left[src_level];
    *upper_margin = upper[src_level];
    *scale = sc[src_level];
    return UGSM_OK;
}

long long ugsm_fovea_cloud_points(int W, int H, int levels, int fovea_levels, int off_x, int off_y, int sampling, long long *per_level)
{
    return ugsm_fovea_multi_cloud_points(W, H, levels, fovea_levels, 1, &off_x, &off_y, sampling, per_level);  // (one window: entry k is level k)
}

int ugsm_triangulate_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, int fovW, int fovH, int src_level,
                           int left_margin, int upper_margin, float scale, const double *P1, const double *P2, float *d_xyz)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!d_stackx || !d_stacky || !P1 || !P2 || !d_xyz || fovW < 1 || fovH < 1 || src_level < 0) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    return timed_launch(ctx, s, slot, (double)fovW * fovH,
                        [&] { launch_triangulate_fovea(s->st, d_stackx, d_stacky, fovW, fovH, src_level, left_margin, upper_margin, scale, P1, P2, d_xyz, ctx_lens(ctx)); });
}

// ---- row f-1, the coloured point cloud (getPointCloud.cpp doReconstructionRGB[_FOV], :615-722) ----------------------------------------

void ugsm_default_cloud_params(ugsm_cloud_params *p)
{
    if (!p) return;
    p->sampling = 1;
    p->format = UGSM_CLOUD_PCL32;
    p->compact = 0;
    p->min_conf = -INFINITY;
    p->z_min = -INFINITY;
    p->z_max = INFINITY;
}

long long ugsm_cloud_points(int W, int H, int sampling)
{
    if (W < 1 || H < 1 || sampling < 1) return -1;
    return (long long)sampled(W, sampling) * sampled(H, sampling);
}

long long ugsm_resized_cloud_points(int W, int H, float factor)
{
    const ResizedGrid g = resized_grid(W, H, factor);
    return g.dw < 1 ? -1 : (long long)g.dw * g.dh;
}

int ugsm_point_cloud(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, const float *d_conf, const uint8_t *d_rgbL, int W, int H,
                     int stride, const double *P1, const double *P2, const ugsm_cloud_params *p, void *d_points, long long cap_points,
                     long long *d_count)
{
    CloudArgs a;
    UCHK(cloud_call_args(ctx, {d_dispx, d_dispy, d_conf, W, H}, {d_rgbL, W, H, stride}, P1, P2, p, {d_points, cap_points, d_count}, a));
    return point_cloud(ctx, slot, a, false, P1, P2);
}

int ugsm_point_cloud_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc, int fovW, int fovH,
                           int src_level, int left_margin, int upper_margin, float scale, const uint8_t *d_rgbL, int W, int H, int stride,
                           const double *P1, const double *P2, const ugsm_cloud_params *p, void *d_points, long long cap_points, long long *d_count)
{
    CloudArgs a;
    UCHK(cloud_call_args(ctx, {d_stackx, d_stacky, d_stackc, fovW, fovH, true, src_level, left_margin, upper_margin, scale}, {d_rgbL, W, H, stride}, P1, P2,
                         p, {d_points, cap_points, d_count}, a));
    return point_cloud(ctx, slot, a, true, P1, P2);
}

// The whole stack as one cloud: level 0, then 1 .. F-1, each without the points the finer level already covers (cloud_stack_table)
int ugsm_point_cloud_fovea_all(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc, int W, int H,
                               int off_x, int off_y, const uint8_t *d_rgbL, int stride, const double *P1, const double *P2,
                               const ugsm_cloud_params *p, void *d_points, long long cap_points, long long *d_count, long long *d_level_counts)
{
    if (!ctx || !p || ((uintptr_t)d_level_counts & 7)) return UGSM_ERR_BAD_ARG;
    CloudStack sk;
    int fw, fh;
    UCHK(cloud_stack_table(W, H, ctx->cfg.levels, ctx->cfg.fovea_levels, off_x, off_y, p->sampling, sk, &fw, &fh));
    CloudArgs a;
    UCHK(cloud_call_args(ctx, {d_stackx, d_stacky, d_stackc, fw, fh}, {d_rgbL, W, H, stride}, P1, P2, p, {d_points, cap_points, d_count}, a));
    sk.level_counts = d_level_counts;
    Slot *s;
    UCHK(cloud_begin(ctx, slot, a, sk.F, &s));
    return timed_launch(ctx, s, slot, (double)sk.F * a.wc * a.hc, [&] { launch_point_cloud_stack(s->st, a, sk, P1, P2, ctx_lens(ctx)); });
}

// The stacks of n windows of one pair as one cloud: the entries level-major, each without what the rule across windows leaves out
// (cloud_multi_entry).  The table goes up on the slot's stream from a page-locked copy; nothing here waits for the stream unless a
// buffer has to grow.
int ugsm_point_cloud_fovea_multi(ugsm_ctx *ctx, int slot, int n, const float *const *d_stack, int W, int H, const int *off_x, const int *off_y,
                                 const uint8_t *d_rgbL, int stride, const double *P1, const double *P2, const ugsm_cloud_params *p, void *d_points,
                                 long long cap_points, long long *d_count, long long *d_entry_counts)
{
    if (!ctx || !p || !d_stack || n < 1 || n > UGSM_MAX_BATCH || ((uintptr_t)d_entry_counts & 7)) return UGSM_ERR_BAD_ARG;
    if (ctx->hooks.lens_set)
        return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_point_cloud_fovea_multi: a lens is set (ugsm_set_lens) and the merged cloud of several windows does not honour it");
    for (int j = 0; j < n; j++)
        if (!d_stack[j]) return UGSM_ERR_BAD_ARG;
    MultiCloud g;
    const int F = ctx->cfg.fovea_levels;
    UCHK(cloud_multi_geometry(W, H, ctx->cfg.levels, F, n, off_x, off_y, p->sampling, g));
    const size_t fn = (size_t)g.fw * g.fh, plane = (size_t)F * fn;
    CloudArgs a;
    UCHK(cloud_call_args(ctx, {d_stack[0], d_stack[0] + plane, d_stack[0] + 2 * plane, g.fw, g.fh}, {d_rgbL, W, H, stride}, P1, P2, p,
                         {d_points, cap_points, d_count}, a));
    a.dx = a.dy = a.conf = nullptr;  // (the planes are the table's, entry by entry)
    Slot *s;
    const int E = g.E;
    CloudEntry *rows;
    UCHK(cloud_begin(ctx, slot, a, E, &s, &rows));
    const bool use_conf = a.compact && p->min_conf > -INFINITY;  // (the confidence planes are read by nothing else)
    long long total = 0;
    for (int e = 0; e < E; e++) {
        cloud_multi_entry(g, e, total, rows[e]);
        const int k = e / n, j = e - k * n;
        rows[e].dx = d_stack[j] + (size_t)k * fn;
        rows[e].dy = rows[e].dx + plane;
        rows[e].conf = use_conf ? rows[e].dx + 2 * plane : nullptr;
        total += rows[e].points;
    }
    UCHK(s->cloud.mc.upload(ctx, s->st, (size_t)E));
    const CloudMulti mu{s->cloud.mc.tab, E, total, d_entry_counts};
    return timed_launch(ctx, s, slot, (double)E * a.wc * a.hc, [&] { launch_point_cloud_multi(s->st, a, mu, P1, P2); });
}

// ---- row f-1, the resized cloud (getPointCloud.cpp doReconstruction_resized / doReconstructionFOV_resized, :724-884) ----------------

int ugsm_point_cloud_resized(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, const float *d_conf, const uint8_t *d_rgbL,
                             int W, int H, int stride, const double *P1, const double *P2, float factor, const ugsm_cloud_params *p,
                             void *d_points, long long cap_points, long long *d_count)
{
    const ResizedGrid g = resized_grid(W, H, factor);
    CloudArgs a;
    UCHK(cloud_call_args(ctx, {d_dispx, d_dispy, d_conf, W, H}, {d_rgbL, W, H, stride}, P1, P2, p, {d_points, cap_points, d_count}, a, &g));
    return point_cloud(ctx, slot, a, false, P1, P2, &g.rz);
}

int ugsm_point_cloud_resized_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc, int fovW,
                                   int fovH, int src_level, int left_margin, int upper_margin, float scale, const uint8_t *d_rgbL, int W, int H,
                                   int stride, const double *P1, const double *P2, float factor, int colour_mapped, const ugsm_cloud_params *p,
                                   void *d_points, long long cap_points, long long *d_count)
{
    const ResizedGrid g = resized_grid(fovW, fovH, factor, colour_mapped);
    CloudArgs a;
    UCHK(cloud_call_args(ctx, {d_stackx, d_stacky, d_stackc, fovW, fovH, true, src_level, left_margin, upper_margin, scale}, {d_rgbL, W, H, stride}, P1, P2,
                         p, {d_points, cap_points, d_count}, a, &g));
    if (colour_mapped != 0 && colour_mapped != 1) return UGSM_ERR_BAD_ARG;
    return point_cloud(ctx, slot, a, true, P1, P2, &g.rz);
}

// ---- row f-1, the depth image (REP 118 32FC1 / 16UC1; the reference's range_map and res_range_map, getPointCloud.cpp:730-758, :813-841) ----

void ugsm_default_depth_params(ugsm_depth_params *p)
{
    if (!p) return;
    p->format = UGSM_DEPTH_32F;
    p->unit = 1.0f;
    p->min_conf = -INFINITY;
    p->z_min = -INFINITY;
    p->z_max = INFINITY;
    p->factor = 1.0f;
}

int ugsm_depth_image_size(int pw, int ph, float factor, int *dw, int *dh)
{
    const ResizedGrid g = resized_grid(pw, ph, factor);
    if (!dw || !dh || g.dw < 1) return UGSM_ERR_BAD_ARG;
    *dw = g.dw;
    *dh = g.dh;
    return UGSM_OK;
}

int ugsm_depth_image(ugsm_ctx *ctx, int slot, const float *d_dispx, const float *d_dispy, const float *d_conf, int W, int H, const double *P1,
                     const double *P2, const ugsm_depth_params *p, void *d_depth, unsigned long long *d_valid)
{
    DepthArgs d;
    UCHK(depth_args_ok(ctx, d_dispx, d_dispy, d_conf, 1, W, H, 1, P1, P2, p, d_depth, d_valid, d));
    const bool u16 = p->format == UGSM_DEPTH_16U;
    return depth_image(ctx, slot, d, 1, [&](hipStream_t st) { launch_depth_image(st, d_dispx, d_dispy, W, H, P1, P2, d, u16, ctx_lens(ctx)); });
}

int ugsm_depth_image_fovea(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc, int W, int H, int off_x,
                           int off_y, int level, const double *P1, const double *P2, const ugsm_depth_params *p, void *d_depth,
                           unsigned long long *d_valid)
{
    if (!ctx || W < 1 || H < 1 || (long long)W * H > kMaxPixels) return UGSM_ERR_BAD_ARG;
    const int F = ctx->cfg.fovea_levels;
    const bool all = level == UGSM_DEPTH_ALL_LEVELS;
    if (F < 2 || (!all && (level < 0 || level >= F))) return UGSM_ERR_BAD_ARG;
    DepthFoveaArgs f{};
    int fw, fh;
    UCHK(fovea_level_mappings(W, H, ctx->cfg.levels, F, off_x, off_y, &fw, &fh, f.lv.left, f.lv.upper, f.lv.scale));
    f.lv.levels = all ? F : 1;
    UCHK(depth_args_ok(ctx, d_stackx, d_stacky, d_stackc, F, fw, fh, f.lv.levels, P1, P2, p, d_depth, d_valid, f.d));
    const bool u16 = p->format == UGSM_DEPTH_16U;
    const int src_level = all ? 0 : level;
    return depth_image(ctx, slot, f.d, f.lv.levels,
                       [&](hipStream_t st) { launch_depth_image_fovea(st, d_stackx, d_stacky, fw, fh, src_level, P1, P2, f, u16, ctx_lens(ctx)); });
}

// The whole frame's image from the stack of a foveated call: what ugsm_reconstruct_full followed by ugsm_depth_image gives, in one launch and
// without the field (k_triangulate's frame forms).
int ugsm_depth_image_fovea_full(ugsm_ctx *ctx, int slot, const float *d_stackx, const float *d_stacky, const float *d_stackc, int W, int H, int off_x,
                                int off_y, const double *P1, const double *P2, const ugsm_depth_params *p, void *d_depth, unsigned long long *d_valid)
{
    return named(ctx, "ugsm_depth_image_fovea_full", [&]() -> int {
        DepthArgs d;
        DepthFrame fr;
        FrameWindow win;
        UCHK(depth_frame_args(ctx, 1, nullptr, d_stackx, d_stacky, d_stackc, W, H, &off_x, &off_y, P1, P2, p, d_depth, d_valid, d, fr, &win));
        return depth_frame(ctx, slot, d_stackx, d_stacky, P1, P2, d, fr, &win, p->format == UGSM_DEPTH_16U);
    });
}

// ... from the stacks of n windows of one pair: what ugsm_reconstruct_full_multi followed by ugsm_depth_image gives
int ugsm_depth_image_fovea_multi(ugsm_ctx *ctx, int slot, int n, const float *const *d_stack, int W, int H, const int *off_x, const int *off_y,
                                 const double *P1, const double *P2, const ugsm_depth_params *p, void *d_depth, unsigned long long *d_valid)
{
    return named(ctx, "ugsm_depth_image_fovea_multi", [&]() -> int {
        if (!d_stack) return UGSM_ERR_BAD_ARG;
        DepthArgs d;
        DepthFrame fr;
        FrameWindow win[UGSM_MAX_BATCH];
        UCHK(depth_frame_args(ctx, n, d_stack, nullptr, nullptr, nullptr, W, H, off_x, off_y, P1, P2, p, d_depth, d_valid, d, fr, win));
        const size_t plane = (size_t)fr.F * fr.fw * fr.fh;
        return depth_frame(ctx, slot, d_stack[0], d_stack[0] + plane, P1, P2, d, fr, win, p->format == UGSM_DEPTH_16U);
    });
}

// ---- lens distortion (include/ugsm.h): the setting, and the definition on the host --------------------------------------------------

// one camera's K (3 x 3, row-major) and D (k1, k2, p1, p2, k3) as the kernels take them; false: a non-finite entry, !(fx > 0) or !(fy > 0)
static bool lens_cam(const double *K, const double *D, LensCam &c)
{
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(K[k])) return false;
    for (int k = 0; k < 5; k++)
        if (!std::isfinite(D[k])) return false;
    if (!(K[0] > 0.0) || !(K[4] > 0.0)) return false;
    c = LensCam{K[0], K[4], K[2], K[5], D[0], D[1], D[2], D[3], D[4]};
    return true;
}
// 0 means the default; false: outside 1 .. 32
static bool lens_iterations(int &iterations)
{
    if (iterations == 0) iterations = 5;
    return iterations >= 1 && iterations <= 32;
}

int ugsm_set_lens(ugsm_ctx *ctx, const double *K1, const double *D1, const double *K2, const double *D2, int iterations)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    const int given = (K1 != nullptr) + (D1 != nullptr) + (K2 != nullptr) + (D2 != nullptr);
    if (given == 0) {  // off
        ctx->hooks.lens_set = false;
        return UGSM_OK;
    }
    if (given != 4) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_set_lens: K1, D1, K2 and D2 are all set or all null");
    Lens ln{};
    if (!lens_cam(K1, D1, ln.cam[0]) || !lens_cam(K2, D2, ln.cam[1]))
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_set_lens: every entry of K and D finite, fx > 0 and fy > 0");
    if (!lens_iterations(iterations)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_set_lens: iterations 1 .. 32 (0: the default, 5)");
    ln.iterations = iterations;
    ctx->lens = ln;
    std::copy(K1, K1 + 9, ctx->lens_K[0]);
    std::copy(K2, K2 + 9, ctx->lens_K[1]);
    ctx->hooks.lens_set = true;
    return UGSM_OK;
}

int ugsm_get_lens(const ugsm_ctx *ctx, double *K1, double *D1, double *K2, double *D2, int *iterations, int *set)
{
    if (!ctx || !set) return UGSM_ERR_BAD_ARG;
    *set = ctx->hooks.lens_set ? 1 : 0;
    if (!ctx->hooks.lens_set) return UGSM_OK;
    double *const K[2] = {K1, K2}, *const D[2] = {D1, D2};
    for (int c = 0; c < 2; c++) {
        const LensCam &m = ctx->lens.cam[c];
        if (K[c]) std::copy(ctx->lens_K[c], ctx->lens_K[c] + 9, K[c]);
        if (D[c]) D[c][0] = m.k1, D[c][1] = m.k2, D[c][2] = m.p1, D[c][3] = m.p2, D[c][4] = m.k3;
    }
    if (iterations) *iterations = ctx->lens.iterations;
    return UGSM_OK;
}

int ugsm_undistort_points(const double *K, const double *D, int iterations, const float *uv_in, float *uv_out, long long n)
{
    LensCam c;
    if (!K || !D || n < 0 || (n > 0 && (!uv_in || !uv_out)) || !lens_cam(K, D, c) || !lens_iterations(iterations)) return UGSM_ERR_BAD_ARG;
    for (long long i = 0; i < n; i++) undistort_point(c, iterations, uv_in[2 * i], uv_in[2 * i + 1], uv_out[2 * i], uv_out[2 * i + 1]);
    return UGSM_OK;
}

}  // extern "C"

// ---- the cloud from the queue (ugsm_enqueue_*_cloud*): a call of n pairs and their clouds -------------------------------------------
// The match goes onto the slot's stream as the batch entry points above put it there (the same helpers in the same order, so the planes are
// the same bits); the clouds follow on the same stream.  A call the matcher runs in lockstep gets ONE cloud launch for its pairs (compact:
// two; launch_point_cloud_batch), from a table uploaded on the stream ahead of it.  A call the matcher runs pair by pair (one pair; the
// full-mode LR check, early exit) gets pair b's cloud behind pair b's match: a managed call of that kind reuses the slot's image and plane
// buffers for every pair.  So does a call whose pairs each evaluate more than kBatchMaxPixels sampled points -- the size above which the
// matcher's own levels go pair by pair, because one pair's launch fills the chip many times over and a batch index buys nothing.
// chk (a call of checked pairs, ugsm_enqueue_full_checked_cloud*; else null): the match is the checked call's -- both directions of the pairs in
// lockstep, one pair too, whatever the context's own LR setting --, the clouds read the checked forward fields, and a managed pair that asks
// for them gets its back planes down beside its forward ones.
// The steps below share the call's plan: what the call is, and what each step has settled for the next.
namespace {
struct CloudPlan {
    const CloudCall *call;
    const CheckedCall *chk;
    int n, W, H, stride, F;
    bool fovea, managed, planes;  // planes: a managed call whose pairs' result planes go down to the host
    bool by_pair;                 // the matcher takes the call pair by pair
    int copies;                   // the pairs the slot's buffers hold at once: one for a managed call that runs pair by pair, n otherwise
    FoveaRoom room;               // a foveated call's states lie at the front of hout
    int fw, fh;                   // the planes the points come from: the fovea window, or the frame
    size_t plane;                 // floats per result plane: the pair's result is three of them
    int step;                     // bytes per record
    int wc, hc;                   // the sampled grid (step 2)
    const uint8_t *dL[UGSM_MAX_BATCH], *dR[UGSM_MAX_BATCH];  // step 1: where every pair's images and result lie on the device
    float *res[UGSM_MAX_BATCH], *back[UGSM_MAX_BATCH];       // back: a checked pair's right-to-left field, where it is taken
    int ox[UGSM_MAX_BATCH], oy[UGSM_MAX_BATCH];              // (foveated calls: the pairs' window offsets)
};

// 1. where every pair's images and result lie on the device
int cloud_call_place(ugsm_ctx *ctx, Slot &s, CloudPlan &q)
{
    const CloudCall &call = *q.call;
    const CheckedCall *chk = q.chk;
    const int n = q.n;
    if (!q.managed) {
        UCHK(s.hout.grow(ctx, q.room.total));
        for (int b = 0; b < n; b++) {
            if (!call.job[b].L || !call.job[b].R || !call.job[b].out) return UGSM_ERR_BAD_ARG;
            q.dL[b] = call.job[b].L;
            q.dR[b] = call.job[b].R;
            q.res[b] = call.job[b].out;
            if (chk) q.back[b] = chk->job[b].back;
        }
        return UGSM_OK;
    }
    // the slot's uploads and hout: [states][results], one result for a call that runs pair by pair, n otherwise; a checked call: [back fields]
    // behind them
    const size_t res_per = (3 * q.plane + 63) & ~(size_t)63, img = ((size_t)q.stride * q.H + 255) & ~(size_t)255;
    UCHK(s.rgb_cap.grow(ctx, img * q.copies, {&s.rgbL, &s.rgbR}));
    bool any_back = false;
    for (int b = 0; chk && b < n; b++) any_back = any_back || chk->job[b].back_planes[0];
    const size_t at_res = q.room.part(q.copies * res_per), at_back = q.room.part(any_back ? q.copies * res_per : 0);
    UCHK(s.hout.grow(ctx, q.room.total));
    for (int b = 0; b < n; b++) {
        const int k = q.by_pair ? 0 : b;
        q.dL[b] = s.rgbL + k * img;
        q.dR[b] = s.rgbR + k * img;
        q.res[b] = s.hout + at_res + k * res_per;
        if (chk && chk->job[b].back_planes[0]) q.back[b] = s.hout + at_back + k * res_per;
    }
    return UGSM_OK;
}

// 2. the table: every pair's cloud arguments, uploaded on the slot's stream; a managed call's clouds and count words; the count buffer
int cloud_call_table(ugsm_ctx *ctx, Slot &s, CloudPlan &q)
{
    SlotCloud &c = s.cloud;
    const ugsm_queue_cloud &spec = *q.call->spec;
    const ugsm_cloud_params &p = spec.params;
    const int n = q.n, F = q.F, entries = q.fovea ? F : 1;
    UCHK(c.cq_tab.grow(ctx, (size_t)kMaxBatch));
    UCHK(c.cq_tab_h.grow(ctx, (size_t)kMaxBatch));
    long long max_cap = 0;
    for (int b = 0; b < n; b++) {
        CloudStack &sk = c.cq_tab_h[b].sk;
        q.ox[b] = q.call->job[b].off_x;
        q.oy[b] = q.call->job[b].off_y;
        long long dense;
        if (q.fovea) {  // (the pair's row of the table gets its stack here, the rest below)
            UCHK(cloud_stack_table(q.W, q.H, ctx->cfg.levels, F, q.ox[b], q.oy[b], p.sampling, sk, nullptr, nullptr));
            dense = sk.lv[F - 1].first + sk.lv[F - 1].points;
        } else {
            dense = ugsm_cloud_points(q.W, q.H, p.sampling);
        }
        c.cq_cap[b] = q.managed ? (spec.max_points > 0 ? std::min(spec.max_points, dense) : dense) : q.call->job[b].cap;
        max_cap = std::max(max_cap, c.cq_cap[b]);
    }
    if (q.managed) {
        c.cq_stride = (size_t)max_cap * q.step;
        UCHK(c.cq_pts.grow(ctx, std::max(c.cq_stride * n, (size_t)16)));
        UCHK(c.cq_words.grow(ctx, kMaxBatch * kCqWords));
        UCHK(c.cq_words_h.grow(ctx, kMaxBatch * kCqWords));
    }
    CloudArgs shape{};  // (what every pair's grid comes from)
    shape.pw = q.fw;
    shape.ph = q.fh;
    shape.s = p.sampling;
    const size_t cnt_per = cloud_grid(ctx, shape, entries).words;  // a pair's region of the count buffer
    q.wc = shape.wc;
    q.hc = shape.hc;
    if (p.compact) UCHK(c.cnt.grow(ctx, cnt_per * n));
    for (int b = 0; b < n; b++) {
        const CloudJob &j = q.call->job[b];
        long long *const words = q.managed ? c.cq_words + b * kCqWords : nullptr, *const levels = q.managed ? words + 1 : j.level_counts;
        const CloudTo to = q.managed ? CloudTo{c.cq_pts + b * c.cq_stride, c.cq_cap[b], words} : CloudTo{j.points, c.cq_cap[b], j.count};
        CloudPair &row = c.cq_tab_h[b];
        UCHK(cloud_call_args(ctx, {q.res[b], q.res[b] + q.plane, q.res[b] + 2 * q.plane, q.fw, q.fh}, {q.dL[b], q.W, q.H, q.stride}, spec.P1, spec.P2, &p, to,
                             row.a));
        if ((uintptr_t)levels & 7) return UGSM_ERR_BAD_ARG;
        cloud_grid(ctx, row.a, entries);
        row.a.cnt = p.compact ? c.cnt + b * cnt_per : nullptr;
        if (q.fovea) row.sk.level_counts = levels;
        else row.sk = CloudStack{};
    }
    HIPCHK(ctx, hipMemcpyAsync(c.cq_tab, c.cq_tab_h, n * sizeof(CloudPair), hipMemcpyHostToDevice, s.st));
    if (p.compact) HIPCHK(ctx, hipMemsetAsync(c.cnt, 0, cnt_per * n * sizeof(unsigned), s.st));  // (the totals of every pair's region)
    return UGSM_OK;
}

// pairs b .. b + k - 1 of the call: one of them, or all in lockstep
int cloud_call_match(ugsm_ctx *ctx, Slot &s, int slot, CloudPlan &q, int b, int k)
{
    if (q.chk) {
        int kept = 0;
        for (int j = b; j < b + k; j++) kept += !q.back[j];
        UCHK(full_checked_bufs(ctx, s, k, kept, q.W, q.H));
        return enqueue_full_checked(ctx, s, slot, k, q.dL + b, q.dR + b, q.W, q.H, q.stride, q.res + b, q.back + b, q.chk->tau);
    }
    return q.fovea ? enqueue_foveated(ctx, s, slot, q.dL + b, q.dR + b, q.W, q.H, q.stride, FoveaCall::pairs(k, q.ox + b, q.oy + b, q.res + b))
                   : enqueue_match_full(ctx, s, slot, k, q.dL + b, q.dR + b, q.W, q.H, q.stride, q.res + b);
}

// a managed pair's planes, and a managed checked pair's back planes, where they are wanted
int cloud_call_download(ugsm_ctx *ctx, Slot &s, const CloudPlan &q, int b)
{
    for (int k = 0; q.planes && k < 3; k++)
        HIPCHK(ctx, hipMemcpyAsync(q.call->job[b].planes[k], q.res[b] + k * q.plane, q.plane * sizeof(float), hipMemcpyDeviceToHost, s.st));
    for (int k = 0; q.managed && q.back[b] && k < 3; k++)
        HIPCHK(ctx, hipMemcpyAsync(q.chk->job[b].back_planes[k], q.back[b] + k * q.plane, q.plane * sizeof(float), hipMemcpyDeviceToHost, s.st));
    return UGSM_OK;
}

// 3. the match, and the clouds behind it; a managed call's count words down behind them
int cloud_call_run(ugsm_ctx *ctx, Slot &s, int slot, CloudPlan &q)
{
    SlotCloud &c = s.cloud;
    const CloudCall &call = *q.call;
    const ugsm_queue_cloud &spec = *call.spec;
    const int n = q.n;
    const size_t img_bytes = (size_t)q.stride * q.H;
    const bool cloud_by_pair = q.by_pair || !batch_level(ctx, (q.fovea ? q.F : 1) * q.wc, q.hc);  // (a pair's sampled points against kBatchMaxPixels)
    if (q.by_pair) {
        for (int b = 0; b < n; b++) {
            if (q.managed) UCHK(stage_in(ctx, s, call.job[b].L, call.job[b].R, q.W, q.H, q.stride));
            UCHK(cloud_call_match(ctx, s, slot, q, b, 1));
            UCHK(cloud_call_download(ctx, s, q, b));
            UCHK(queue_cloud_launch(ctx, s, slot, b, 1, q.fovea, &spec));
        }
    } else {
        if (q.managed)
            for (int b = 0; b < n; b++) {
                HIPCHK(ctx, hipMemcpyAsync(const_cast<uint8_t *>(q.dL[b]), call.job[b].L, img_bytes, hipMemcpyHostToDevice, s.st));
                HIPCHK(ctx, hipMemcpyAsync(const_cast<uint8_t *>(q.dR[b]), call.job[b].R, img_bytes, hipMemcpyHostToDevice, s.st));
            }
        UCHK(cloud_call_match(ctx, s, slot, q, 0, n));
        for (int b = 0; b < n; b++) UCHK(cloud_call_download(ctx, s, q, b));
        if (cloud_by_pair)
            for (int b = 0; b < n; b++) UCHK(queue_cloud_launch(ctx, s, slot, b, 1, q.fovea, &spec));
        else
            UCHK(queue_cloud_launch(ctx, s, slot, 0, n, q.fovea, &spec));
    }
    if (q.managed) {
        HIPCHK(ctx, hipMemcpyAsync(c.cq_words_h, c.cq_words, n * kCqWords * sizeof(long long), hipMemcpyDeviceToHost, s.st));
        c.cq_n = n;
        c.cq_step = q.step;
        c.cq_levels = q.fovea ? q.F : 0;
    }
    return mark_done(ctx, s);
}
}  // namespace

static int cloud_call_submit(ugsm_ctx *ctx, int slot, const CloudCall *call, const CheckedCall *chk)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!call || !call->spec || call->n < 1 || call->n > UGSM_MAX_BATCH) return UGSM_ERR_BAD_ARG;
    CloudPlan q{};
    q.call = call;
    q.chk = chk;
    q.n = call->n;
    q.W = call->W;
    q.H = call->H;
    q.stride = call->stride;
    q.F = ctx->cfg.fovea_levels;
    q.fovea = call->fovea != 0;
    q.managed = call->managed != 0;
    q.planes = q.managed && call->spec->want_planes != 0;
    if (q.fovea && q.F < 2) return UGSM_ERR_BAD_ARG;
    if (q.W < 1 || q.H < 1) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < q.n; b++) UCHK(input_status(ctx, q.W, q.stride, call->job[b].L, call->job[b].R));
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    s->cloud.cq_n = 0;
    if (chk) UCHK(full_checked_check(ctx, q.n, q.W, q.H, q.stride, chk->tau));
    q.by_pair = q.n == 1 || (!chk && (q.fovea ? fovea_batch_runs_pair_by_pair(ctx) : batch_runs_pair_by_pair(ctx)));
    q.copies = q.managed && q.by_pair ? 1 : q.n;
    if (q.fovea) UCHK(fovea_room(ctx, q.W, q.H, FoveaCall::Pairs, q.copies, q.room));
    q.fw = q.fovea ? q.room.fw : q.W;
    q.fh = q.fovea ? q.room.fh : q.H;
    q.plane = q.fovea ? q.room.plane : (size_t)q.W * q.H;
    q.step = call->spec->params.format == UGSM_CLOUD_PCL32 ? 32 : 16;
    UCHK(cloud_call_place(ctx, *s, q));
    UCHK(cloud_call_table(ctx, *s, q));
    return cloud_call_run(ctx, *s, slot, q);
}

int ugsm::queue_cloud_submit(ugsm_ctx *ctx, int slot, const CloudCall *call) { return cloud_call_submit(ctx, slot, call, nullptr); }

// The checked call's pairs with a cloud each (CtxHooks::checked_submit hands them on from ugsm_full.cpp): the same call as a cloud call of
// full-mode pairs, with the checked match in the place of the plain one.
int ugsm::queue_checked_cloud_submit(ugsm_ctx *ctx, int slot, const CheckedCall *chk)
{
    if (!chk || !chk->spec || chk->n < 1 || chk->n > UGSM_MAX_BATCH) return UGSM_ERR_BAD_ARG;
    CloudCall cc{0, chk->managed, chk->n, chk->W, chk->H, chk->stride, chk->spec, {}};
    for (int b = 0; b < chk->n; b++) {
        const CheckedJob &j = chk->job[b];
        cc.job[b] = CloudJob{j.L, j.R, 0, 0, j.out, {j.planes[0], j.planes[1], j.planes[2]}, j.points, j.cap, j.count, nullptr};
    }
    return cloud_call_submit(ctx, slot, &cc, chk);
}

int ugsm::queue_cloud_finish(ugsm_ctx *ctx, int slot, int n, ugsm_cloud_result *res, void *(*staging)(void *, int, long long), void *user)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    SlotCloud &c = s->cloud;
    if (!res || !staging || n < 1 || n != c.cq_n) return ctx_fail(ctx, UGSM_ERR_STATE, "the slot holds no managed cloud call of that many pairs");
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    for (int b = 0; b < n; b++) {
        const long long *w = c.cq_words_h + b * kCqWords;
        ugsm_cloud_result &r = res[b];
        r = ugsm_cloud_result{};
        r.count = w[0];
        r.stored = std::min(w[0], c.cq_cap[b]);
        r.point_step = c.cq_step;
        r.levels = c.cq_levels;
        for (int l = 0; l < c.cq_levels; l++) r.level_counts[l] = w[1 + l];
    }
    c.cq_n = 0;
    for (int b = 0; b < n; b++) {
        if (res[b].stored < 1) continue;
        const long long bytes = res[b].stored * c.cq_step;
        res[b].points = staging(user, b, bytes);
        if (!res[b].points) return ctx_fail(ctx, UGSM_ERR_NOMEM, "no page-locked memory for a pair's cloud");
        HIPCHK(ctx, hipMemcpyAsync(res[b].points, c.cq_pts + b * c.cq_stride, (size_t)bytes, hipMemcpyDeviceToHost, s->st));
    }
    return mark_done(ctx, *s);
}
