// ugsm_launch.hpp -- host-visible launchers of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>

namespace ugsm {

// Per-launch timing (ugsm_config.profile_events): when the submitting thread has a probe set, the next launch carries the probe's two
// events IN its dispatch (hipExtLaunchKernelGGL: the kernel's own begin and end timestamps, what rocprofv3's kernel trace reports), not
// two hipEventRecord markers around it, whose interval also holds the gaps to the neighbouring launches (6 us per launch on this stack:
// 8 % of the dominant kernel's mean duration; profiles/r04_trace_summary.md).  Almost every bracket of the runtime holds ONE launch; where
// a bracket holds several (the development fallback of launch_blur_decimate: reference kernel + range scan), the first launch carries
// the start event and every launch re-records the stop event, so the interval runs from the first kernel's begin to the LAST kernel's
// end and no launch of the bracket goes untimed; n counts them.
struct LaunchProbe {
    hipEvent_t a, b;
    int n;
};
inline thread_local LaunchProbe *g_probe = nullptr;
#define UGSM_LAUNCH(kern, grid, block, shmem, st, ...)                                                                \
    do {                                                                                                              \
        ::ugsm::LaunchProbe *probe_ = ::ugsm::g_probe;                                                                \
        if (probe_) hipExtLaunchKernelGGL(kern, grid, block, shmem, st, probe_->n++ == 0 ? probe_->a : nullptr, probe_->b, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, grid, block, shmem, st, __VA_ARGS__);                                           \
    } while (0)

// A 3-plane float image view: plane k starts at p + k*plane, rows are `pitch` floats
// apart.  Pyramid levels are dense (pitch == width); fovea crops of the pyramid
// (CreateFoveatedPyramid, MatchGPULib.cpp:1171-1185) are views into the full level,
// not copies -- kernels clamp / zero-pad at the view's logical W x H.
struct Img3 {
    const float *p;
    int pitch;
    size_t plane;
};
// Level 0 of a full-mode call is the camera image itself: (float) of its bytes, never stored.  The kernels that read level 0 take the image
// in an Img3 -- p the interleaved 8-bit image, pitch its row stride in BYTES, plane unused -- together with its InLayout (`in`).
// K-cost and K-sq are templates on that input form: kInPlanes -- the float planes of a pyramid level -- or kInRGB8 (InLayout, ugsm_device.hpp: 0),
// the one 8-bit layout they are instantiated for.  The launchers take it as `in` and refuse any other value.
constexpr int kInPlanes = -1;
inline Img3 byte_view(const uint8_t *image, int stride) { return Img3{reinterpret_cast<const float *>(image), stride, 0}; }

// Where a level's first iteration finds its starting field when the seeding is fused into K-cost: the coarser level's
// (dx, dy, conf), Ws x Hs, sampled as subsampleDispKernel does (MatchLib.cu:372-401) with the fovea crop offset (cx, cy).
struct SeedMap {
    int Ws, Hs, cx, cy;
};

// B pairs of ONE size in one launch (round 4: the batch dimension).  Every launch of a level of 615 x 407 pixels and below lasts as long
// as one tile's or one strip's chain, whatever the chip could do beside it; with B pairs marching through the levels in lockstep the
// same launch carries B times the work: gridDim.y (gridDim.z / 3 where y is the image row) = pairs, and the kernel shifts its pointers
// to its pair's planes before it does anything else.  Offsets are BYTES relative to the pointers of the launch, which are pair 0's.
constexpr int kMaxBatch = 16;  // = UGSM_MAX_BATCH (include/ugsm.h)
struct Batch {
    int n;                     // pairs in the launch; <= 1: one pair, nothing below is read
    int cx[kMaxBatch], cy[kMaxBatch];  // seeded launches: SeedMap.cx / cy of pair b (fovea windows of different pairs sit at different places)
    long long img[kMaxBatch];  // pair b's image planes: the L and R views (K-cost, A = G * L^2), the rgb8 image (k_pyr_base), a level of the pyramid (k_blur_decimate, k_copy_view)
    long long in[kMaxBatch];   // pair b's input fields: d3 / coarse3 / s3, and A3
    long long out[kMaxBatch];  // pair b's output: nd3 / o3 / dst (a slot buffer, or the caller's)
};

// ---- plain per-pixel kernels (ugsm_kernels_aux.hip, _fields.hip, _depth.hip, _cloud.hip, _warp.hip) ----
void launch_seed(hipStream_t st, const float *src3, int Ws, int Hs, float *dst3, int Wd, int Hd, int cx, int cy, const Batch *bt = nullptr);
// The restriction, k_restrict (ugsm_submit_full_seeded): level `level`'s starting field dst3 (w x h, the level's size) from the
// full-resolution field src3 (W x H).  Batched: pair b reads src3 + bt->in[b] bytes and writes dst3 + bt->out[b] bytes.
struct RestrictMap {
    int W, H, w, h, k, odd;  // k = level / 2, odd = level & 1
    float scale;             // 2^-k
};
void launch_restrict(hipStream_t st, const float *src3, int W, int H, int level, float *dst3, int w, int h, const Batch *bt = nullptr);
void launch_copy_view(hipStream_t st, Img3 src, int W, int H, float *dst, size_t dst_plane, int dst_pitch, const Batch *bt = nullptr);
// The prolongation, k_prolong (ugsm_submit_full_coarse, ugsm_stage_prolong): the field src3 of level `level` (3 planes of w[level] x
// h[level]) at full resolution in dst3 (3 planes of w[0] x h[0]), as `level` steps of k_seed give it, in one launch.  w, h: the sizes of the
// levels 0 .. level (ugsm_level_dims); every level's own size takes part (its clamp).  Batched: pair b reads src3 + bt->in[b] bytes and
// writes dst3 + bt->out[b] bytes.  False (nothing launched): a level or a size the kernel's bounds do not cover.
constexpr int kProlongMaxLevels = 32;  // = UGSM_MAX_LEVELS (include/ugsm.h)
struct ProlongMap {
    int W, H, ws, hs;  // the output's size and the state's
    int e, vec;        // the state's level; pixels per store: 4, 2 or 1, what every row's alignment allows
    int w[kProlongMaxLevels], h[kProlongMaxLevels];  // the sizes of the levels 0 .. e
};
bool launch_prolong(hipStream_t st, const float *src3, const int *w, const int *h, int level, float *dst3, const Batch *bt = nullptr);
// rgb8 -> planar float level 0 (MatchGPULib.cpp:332-338) where k_pyr_base does not apply: pyramids of fewer than three levels, kernel_path 1
void launch_rgb_planes(hipStream_t st, const uint8_t *rgb, int stride, int W, int H, float *planes, int fmt = 0);
// Level 0 of one pair inside n fovea windows of w x h level-0 pixels at (x0[k], y0[k]) -- k_level0_windows, one launch for both
// images (ugsm_submit_foveated_multi: the pyramid pass stores no level 0 there, kPyrNoLevel0).  planesL / planesR: the two level-0 planes
// (W x H each).  The four-byte formats take their word loads when both images and the stride are 4-byte aligned.  False (nothing launched): a
// window that leaves the frame.
struct Level0Windows {
    int n, w, h;
    int x0[kMaxBatch], y0[kMaxBatch];
};
bool launch_level0_windows(hipStream_t st, const uint8_t *rgbL, const uint8_t *rgbR, int stride, int W, int H, float *planesL, float *planesR,
                           const Level0Windows &win, int fmt = 0);
// LR-consistency check (north_star; no reference counterpart): zeroes the confidence of left3 where right3 does not point back within tau
void launch_lr_check(hipStream_t st, float *left3, const float *right3, int W, int H, float tau, unsigned long long *marked);
// The stack form (a checked foveated call, ugsm_set_lr_check): every level of the fovea stacks of n pairs in ONE launch, grid.z = pair x F +
// level.  A stack is 3 x (F fovH) x fovW floats (plane p of level k at (p F + k) fovW fovH); level k of pair b's left-to-right stack
// (stack0 + fwd[b] bytes: the caller's buffer) is checked against level k of its right-to-left stack (back0 + back[b] bytes: the slot's)
// by the rule above, on the level's own fovW x fovH grid.  marked[b * F + k] counts the pixels marked (zeroed by the caller).
struct LrStack {
    int n, F;
    long long fwd[kMaxBatch], back[kMaxBatch];
};
void launch_lr_check(hipStream_t st, float *stack0, const float *back0, int fovW, int fovH, float tau, unsigned long long *marked, const LrStack &ls);
// (F = 1: a stack is one full-frame field.  A checked full-mode call, ugsm_submit_full_checked, checks both directions of its pairs so: entry
// 2 b = pair b's left-to-right field against its right-to-left one, entry 2 b + 1 the two exchanged, both pointers relative to one base.)
// X, Y, Z planes from the full-resolution (dx, dy) and the two 3x4 projection matrices
// lens (here and in every launcher below that takes one; ugsm_lens.hpp): null -- the pixel positions are pinhole coordinates, the instances
// that have always been launched; else the launch's lens form, which takes the Lens by value behind the same arguments and undistorts both
// positions of every correspondence just before the closed form.
struct Lens;
void launch_triangulate(hipStream_t st, const float *dispx, const float *dispy, int W, int H, const double *P1, const double *P2, float *xyz,
                        const Lens *lens = nullptr);
void launch_triangulate_fovea(hipStream_t st, const float *stackx, const float *stacky, int fovW, int fovH, int src_level, int left_margin,
                              int upper_margin, float scale, const double *P1, const double *P2, float *xyz, const Lens *lens = nullptr);
// SURVEY 8f row f-1, the coloured point cloud (ugsm_point_cloud[_fovea]): k_cloud[_fovea]<kTriCloudCount / kTriCloud>.
// The sampled grid is wc x hc points (point (ci, cj) = pixel (ci * s, cj * s) of the planes); tiles of 32 columns x 64 rows of it.
struct CloudArgs {
    const float *dx, *dy, *conf;  // pw x ph row-major planes (the fovea form: level src_level of the stacks); conf may be null
    int pw, ph;
    const uint8_t *rgb;           // the left image, W x H, `stride` bytes per row, in input format fmt
    int W, H, stride;
    int s, wc, hc, nchunk;        // sampling; the sampled grid; cloud_chunks(hc)
    int format, compact;          // UGSM_CLOUD_PCL32 (0) / UGSM_CLOUD_XYZRGB16 (1); compact: only the points that pass the filter
    float min_conf, z_min, z_max;
    int left_margin, upper_margin;  // the fovea form: mapXcoord / mapYcoord (ugsm_fovea_mapping)
    float scale;
    int fmt;        // the input format of rgb (UGSM_INPUT_*)
    unsigned *cnt;  // compact: wc * nchunk counts, wc column totals, cloud_strips(wc) strip totals; the totals zeroed before the launch
    void *points;   // 16-byte aligned
    long long cap;
    long long *count;
};
// the resized cloud (ugsm_point_cloud_resized[_fovea]): k_cloud[_fovea]<kTriResizedCount / kTriResized>, whose grid is the resized map
// (CloudArgs.wc x hc = (int)(pw * factor) x (int)(ph * factor), s 1): point (ci, cj) = pixel (ci, cj) of it
struct CloudResize {
    double scale_x, scale_y;  // cv::resize's 1. / ((double)wc / pw), 1. / ((double)hc / ph)
    float factor;
    int same_size;            // wc == pw && hc == ph: cv::resize copies, Z is the pixel's own
    int colour_mapped;        // the fovea form: the colour at the mapped pixel (as ugsm_point_cloud_fovea) rather than at (xx, yy)
};
// the merged cloud of the whole fovea stack (ugsm_point_cloud_fovea_all): k_cloud_stack<kTriStackCount / kTriStack>, whose grid runs over
// F * cloud_strips(wc) strips (level = strip / strips).  CloudArgs.dx / dy / conf are the stacks (level 0's planes); a workgroup takes its
// level's planes, mapping and covered rectangle from its row of the table.  A pixel of level k >= 1 whose footprint lies wholly inside
// level k-1's window is covered and left out (include/ugsm.h); the rule is separable and monotone, so the host hands over one interval
// of sampled columns and one of sampled rows per level.
struct CloudLevel {
    long long plane;   // the level's planes inside the stacks, in floats
    long long first;   // dense: the level's first record
    long long points;  // dense: the level's records, wc * hc - (cx1 - cx0) * (cy1 - cy0)
    int left_margin, upper_margin;  // ugsm_fovea_level_mapping
    float scale;
    int cx0, cx1, cy0, cy1;  // the covered sampled columns [cx0, cx1) and rows [cy0, cy1); nothing covered: all 0
};
constexpr int kCloudMaxLevels = 32;  // = UGSM_MAX_LEVELS (include/ugsm.h)
struct CloudStack {
    int F, strips;             // fovea levels; cloud_strips(wc)
    long long *level_counts;   // F entries, may be null
    CloudLevel lv[kCloudMaxLevels];
};
int cloud_strips(int wc);
int cloud_chunks(int hc);
// compact: a count launch, then the cloud launch; dense: the cloud launch.  rz: the resized forms
void launch_point_cloud(hipStream_t st, const CloudArgs &args, bool fovea, const double *P1, const double *P2, const CloudResize *rz = nullptr,
                        const Lens *lens = nullptr);
// the same for the merged cloud of the stack; args.cnt (compact): (F * wc) * nchunk counts, F * wc column totals, F * strips strip totals
void launch_point_cloud_stack(hipStream_t st, const CloudArgs &args, const CloudStack &sk, const double *P1, const double *P2,
                              const Lens *lens = nullptr);
// The clouds of the n pairs of a queue call in ONE launch (compact: two), the pair = blockIdx.z: k_cloud_pairs / k_cloud_stack_pairs read their
// pair's row of a table in DEVICE memory instead of kernel arguments (sixteen CloudStacks do not fit there).  Every row holds the pair's
// whole CloudArgs -- its planes or stack, image, its own region of the count buffer (zeroed before the launch), points, cap and count --
// and, for k_cloud_stack_pairs, its own CloudStack: windows at different offsets have different margins and covered rectangles.  The pairs
// share everything that shapes the grid (pw, ph, s, compact; F and strips), which `shape` (a host copy of any row) gives.
struct CloudPair {
    CloudArgs a;
    CloudStack sk;
};
void launch_point_cloud_batch(hipStream_t st, const CloudPair *d_table, int n, const CloudPair &shape, bool stack, const double *P1, const double *P2);
// The merged cloud of the stacks of n windows of ONE pair (ugsm_point_cloud_fovea_multi): k_cloud_multi<kTriMultiCount / kTriMulti>, whose grid
// runs over E * cloud_strips(wc) strips, E = (F-1) n + 1 entries (entry = strip / strips).  A workgroup takes its entry's row of a table
// in DEVICE memory (E reaches 97 and a row holds up to 31 rectangles: no room among the kernel arguments): the entry's planes and mapping,
// the rectangles of its sampled grid that the rule across windows leaves out (include/ugsm.h; a union, so they may overlap), and what the
// dense offsets need -- the entry's first record, and the columns cut into segments at the rectangles' edges: inside a segment every
// column keeps the same number of rows, so a column's first record is its segment's plus a product.
constexpr int kCloudMaxRects = 2 * kMaxBatch - 1;     // n windows' finer levels + the n - 1 higher-numbered windows' same level
constexpr int kCloudMaxSegs = 2 * kCloudMaxRects + 1;
struct CloudRect {
    int cx0, cx1, cy0, cy1;  // the sampled columns [cx0, cx1) and rows [cy0, cy1); never empty
};
struct CloudEntry {
    const float *dx, *dy, *conf;    // the entry's level of its stack
    int left_margin, upper_margin;  // ugsm_fovea_level_mapping for the entry's window
    float scale;
    int nrect, nseg;
    long long first, points;        // dense: the entry's first record and its records
    CloudRect rect[kCloudMaxRects];
    int seg_x[kCloudMaxSegs];           // segment g = the columns from seg_x[g] up to the next segment's (the last: up to wc)
    int seg_rows[kCloudMaxSegs];        // the rows each of its columns keeps
    unsigned seg_first[kCloudMaxSegs];  // the entry's records before its first column
};
struct CloudMulti {
    const CloudEntry *table;  // device memory, E rows
    int E;
    long long total;          // dense: the cloud's size
    long long *entry_counts;  // E entries, may be null
};
// args.dx / dy / conf are not read (the table's are); args.cnt (compact): (E * wc) * nchunk counts, E * wc column totals, E * strips strip totals
void launch_point_cloud_multi(hipStream_t st, const CloudArgs &args, const CloudMulti &mu, const double *P1, const double *P2);
// The depth image (ugsm_depth_image[_fovea]; REP 118): the Z of k_triangulate[_fovea], or the resized clouds' Z, as a row-major image of
// 32FC1 / 16UC1 elements -- the depth forms of those two kernels.  The image of a level is dw x dh (factor 1: the planes' pw x ph, indexed
// flat: a thread owns a run of 16 bytes of adjacent pixels, the first run starting where the image is 16-byte aligned; factor < 1:
// CloudResize's map, a thread a pixel).  The fovea form takes `levels` levels from src_level on in one launch (the grid's y), each mapped by
// its row of the table (ugsm_fovea_level_mapping), images and counts level after level.
struct DepthArgs {
    const float *conf;          // the confidence plane (the fovea form: the stack's, level 0 first); null: no confidence test
    void *out;                  // dw * dh elements a level: float (32F) or uint16_t (16U), aligned to the element
    unsigned long long *valid;  // the valid pixels stored, a count a level, zeroed before the launch; may be null
    float unit, min_conf, z_min, z_max;
    int dw, dh;
    CloudResize rz;             // the resized forms (factor < 1)
};
struct DepthLevels {
    int levels;                 // the launch's levels: src_level .. src_level + levels - 1
    int left[kCloudMaxLevels], upper[kCloudMaxLevels];
    float scale[kCloudMaxLevels];
};
struct DepthFoveaArgs {
    DepthArgs d;
    DepthLevels lv;
};
// u16: UGSM_DEPTH_16U, else UGSM_DEPTH_32F; d.rz.factor < 1: the resized form
void launch_depth_image(hipStream_t st, const float *dispx, const float *dispy, int W, int H, const double *P1, const double *P2, const DepthArgs &d,
                        bool u16, const Lens *lens = nullptr);
void launch_depth_image_fovea(hipStream_t st, const float *stackx, const float *stacky, int fovW, int fovH, int src_level, const double *P1,
                              const double *P2, const DepthFoveaArgs &d, bool u16, const Lens *lens = nullptr);
// The depth image of the WHOLE frame from a fovea stack (ugsm_depth_image_fovea_full / _multi): the frame forms of k_triangulate, the depth forms above over the
// W x H frame (DepthArgs.dw x dh its image) with another source of a pixel's (dx, dy, conf) -- not a read of a full-resolution plane but the
// value ugsm_reconstruct_full[_multi] would have put there, found per pixel as k_restrict_stack finds it: descend from level 0 until a
// level's window holds the site (several windows: the highest-numbered one that does; level F-1 holds every site and is stack 0's), then as
// many multiplications by (float)1.41421356 as levels were descended, every channel.  The field is never formed.
// A window = its origin at every level l < F-1 and its stack's distance from stack 0 in BYTES (the three plane pointers of the launch are
// stack 0's and every window's planes lie the same distance behind them).  One window travels in the kernel arguments; n > 1 are read from
// `table`, n rows in DEVICE memory (sixteen do not fit among the arguments: kRestrictStackByValue, below).
struct FrameWindow {
    long long stack;
    int ox[kCloudMaxLevels], oy[kCloudMaxLevels];
};
struct DepthFrame {
    int n, F, fw, fh;                            // windows; fovea levels; a level's window (w[F-1] x h[F-1] = fw x fh)
    int w[kCloudMaxLevels], h[kCloudMaxLevels];  // the sizes of the levels 0 .. F-1 (w[0] x h[0] = the frame)
    const FrameWindow *table;                    // n > 1: the windows, in device memory; else null and `win` is the window
    FrameWindow win;
};
// stackx / stacky: the dx and dy planes of stack 0 (F x fh x fw floats each), d.conf its confidence plane or null.  win: the n windows in HOST
// memory -- checked here (n = 1: copied into the arguments; n > 1: they must be what fr.table holds).  False (nothing launched): a shape the
// kernel's bounds do not cover -- a window that leaves its level, sizes that do not fit together, n > 1 without a table.
bool launch_depth_image_frame(hipStream_t st, const float *stackx, const float *stacky, const double *P1, const double *P2, const DepthArgs &d,
                              DepthFrame fr, const FrameWindow *win, bool u16, const Lens *lens = nullptr);
void launch_upsample_paste(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, const float *fovH_, const float *fovV_,
                           const float *fovC_, int fovW, int fovH, int org_x, int org_y);
// The same step with the fovea of n stacks of one pair (ugsm_reconstruct_full_multi): window k's crop origin at this level, and its stack's
// distance from stack 0 in BYTES.  fov0: this level's dx plane in stack 0; dy and conf lie fov_plane, 2 fov_plane floats behind it.
struct PasteWindows {
    int n;
    int org_x[kMaxBatch], org_y[kMaxBatch];
    long long stack[kMaxBatch];
};
void launch_upsample_paste_multi(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, const float *fov0, size_t fov_plane,
                                 int fovW, int fovH, const PasteWindows &pw);
// The same rule POINTWISE, k_restrict_stack (the warm foveated call, ugsm_submit_foveated_warm): the starting
// fields of the fovea levels s .. F-1 of n entries from a prior each, in ONE launch, grid.z = entry x (F - s) + (level - s).  The field of
// level k is the fw x fh crop, at the NEW window's origin at level k, of the restriction (RestrictMap, above) to level k of the full-resolution
// field that ugsm_reconstruct_full gives for the prior stack -- computed per target pixel: the pixel's level-0 site, then the paste rule
// descended from level 0 of the prior stack until a level's window holds the site (level F-1 holds every site), then as many multiplications
// by (float)1.41421356 as levels were descended.  Neither the full-resolution field nor its restriction is ever formed.
// A row = one entry: where its prior and its destinations lie (BYTES relative to the launch's pointers) and the two windows' origins.
// field != 0: the priors are full-resolution fields (3 planes of W x H) and the descent has depth zero; pox / poy are not read.
// Destinations: level k > s, and level s where work0 is null, go to row block k of the entry's stack (3 planes of F x fh x fw) at stack0 + dst;
// with work0, level s goes to the 3 dense planes of fw x fh at work0 + work (the level buffer the matching starts in).
// Up to kRestrictStackByValue rows travel in the kernel arguments (sixteen do not fit there); more are read from `table`, n rows in DEVICE memory.
struct RestrictStackRow {
    long long prior, dst, work;
    int nox[kCloudMaxLevels], noy[kCloudMaxLevels];  // the new window's origin at level k (k = F-1: 0, the whole level)
    int pox[kCloudMaxLevels], poy[kCloudMaxLevels];  // the prior's window at level l < F-1
};
constexpr int kRestrictStackByValue = 2;
struct RestrictStack {
    int n, F, s, field;
    int W, H, fw, fh;
    int w[kCloudMaxLevels], h[kCloudMaxLevels];  // the sizes of the levels 0 .. F-1 (w[F-1] x h[F-1] = fw x fh)
    const RestrictStackRow *table;               // null: rows[] below
    RestrictStackRow rows[kRestrictStackByValue];
};
// rows: the n rows in HOST memory -- checked here, and copied into the arguments where rs.table is null (rs.rows is the launcher's to fill).
// False (nothing launched): a shape the kernel's bounds do not cover (a window that leaves its level, more rows by value than there is room for).
bool launch_restrict_stack(hipStream_t st, const float *prior0, float *stack0, float *work0, RestrictStack rs, const RestrictStackRow *rows);
// S_dx, S_dy, C of weightedDifference (MatchGPULib.cpp:1336-1437) into out3; rowsum = 3*H doubles of scratch
void launch_weighted_difference(hipStream_t st, const float *newd3, const float *oldd3, int W, int H, double *rowsum, double *out3);
// MatchGPULib::warpRightImage (MatchGPULib.cpp:1445-1518, kernel warpAbyB MatchLib.cu:499-549) -- k_warp_right:
//   dst[iy][ix] = src[tex_index(((float)iy + 0.5f) + dy[iy][ix], H)][tex_index(((float)ix + 0.5f) + dx[iy][ix], W)], the value stored as fetched.
// in == kInPlanes: src is `planes` float planes of W x H, dst as many, the grid's z the plane; plane z is warped by field z / per_field of
// dx / dy (fields W x H apart): per_field = planes for one field for all of them, 3 for a fovea stack (z = 3 x level + channel).
// in == an input format (UGSM_INPUT_*): src is the 8-bit image (`stride` bytes a row), planes == 3: a thread fetches its pixel once and
// stores the three (the four-byte formats take their word loads where the image and the stride are 4-byte aligned).
struct WarpArgs {
    const void *src;
    int stride, W, H, planes, per_field;
    const float *dx, *dy;
    float *dst;
};
void launch_warp(hipStream_t st, const WarpArgs &a, int in);
// The photometric residual of a match -- k_residual_rows / k_residual_total: per channel c, t = fabsf(L_c - warp(R_c)) in float, t = t * conf in
// float, S_c = sum(t), C = sum(conf) (conf null: 1.0f), binary64 sums in row f-4's fixed order.  in == kInPlanes: L and R are `levels` levels of
// [channel][row] float planes (a fovea pyramid stack), dx / dy / conf as many levels of W x H; an input format (UGSM_INPUT_*): the two 8-bit images, levels == 1.
// rowsum: levels x H x 4 doubles of scratch; sums: levels x 4 doubles [S0, S1, S2, C].  Two launches for all levels.
struct ResidualArgs {
    const void *L, *R;
    int stride, W, H, levels;
    const float *dx, *dy, *conf;
    double *rowsum;
};
void launch_residual(hipStream_t st, const ResidualArgs &a, int in, double *sums);

// ---- libugsm_dev.so only (csrc/dev/): kernel_path 1 (one kernel per reference stage), round 1's LDS-tiled K-cost
// (ugsm_config.march_min_pixels < 0) and the probe kernels.  The product links no-op stand-ins (ugsm_no_dev.cpp) so that the runtime is the
// same objects in both libraries; ugsm_create refuses the configurations that would reach them, the kernel-choice policy gives every other level
// a shipped K-cost form (run_level answers UGSM_ERR_STATE rather than reach launch_cost_fused here) and the probe entry points
// (dev/ugsm_dev_entries.cpp) are not linked in.  kDevLib: which of the two a library is, defined by the file only it links.
extern const bool kDevLib;
void launch_blur_decimate_ref(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, float sf);
void launch_sqblur_clamp_ref(hipStream_t st, Img3 src, int W, int H, float *dst3);
void launch_warp_ref(hipStream_t st, Img3 R, const float *d3, int W, int H, float *Rw3);
void launch_cost_ref(hipStream_t st, Img3 L, const float *Rw3, const float *A3, const float *B3, const float *d3, float *nd3,
                     int W, int H, float thr, int blend, float *dbg8);
void launch_smooth_pass_ref(hipStream_t st, const float *s3, float *o3, int W, int H);
void launch_box_ref(hipStream_t st, const float *s3, float *o3, int W, int H);
// One iteration's warp + cost + parabola + update, LDS-tiled (k_cost_split; no batch index)
void launch_cost_fused(hipStream_t st, Img3 L, Img3 R, const float *A3, const float *d3, float *nd3, int W, int H, float thr, int blend);
// test hooks: the product kernels' exact shortcuts (range-guarded division, shared-reciprocal division, parabola fast path, x/3) on arbitrary operands
void launch_div_probe(hipStream_t st, const float *n, const float *d, float *q, int count);
void launch_div3_probe(hipStream_t st, const float *a0, const float *a1, const float *a2, const float *s, float *q0, float *q1, float *q2, int n);
void launch_poly_probe(hipStream_t st, const float *c, const float *l, const float *r, const float *thr, float *delta, float *corr, float *third, int n);

// ---- K-cost ----------------------------------------------------------------------------------
// One iteration's warp + cost + parabola + update as a marching kernel (ugsm_kernels_march.hip): one wave per strip of columns, no LDS.
// rows = strip height (> 0 fixed; 0 / -1 / -2 / -3: launch_cost_march_t's modes).
// in: kInPlanes -- L and R are float planes; kInRGB8 -- byte_view()s of the rgb8 images (level 0 of a full-mode call).  A batched launch of the
// latter carries pair b's R image offset in bt->cx[b] (low word) and bt->cy[b] (high word): the two images of a pair are unrelated pointers and
// Batch::img holds one offset.  Those fields are the seed-crop origins of the float form, so the rgb8 form takes every origin as ZERO -- true of
// full mode, its only user; run_level refuses anything else.  (A field of its own would move the kernel arguments behind Batch in every kernel
// that takes one -- k_pyr_base's window among them -- for one launch per pair.)
void launch_cost_march(hipStream_t st, Img3 L, Img3 R, const float *A3, const float *d3, float *nd3, int W, int H, float thr, int blend, int rows,
                       const unsigned *range_bad, const Batch *bt = nullptr, int in = kInPlanes);
// First iteration of a level with the seeding fused in: coarse3 = the coarser level's field (never materialised at this level's size)
void launch_cost_march_seeded(hipStream_t st, Img3 L, Img3 R, const float *A3, const float *coarse3, SeedMap sm, float *nd3, int W, int H, float thr,
                              int blend, int rows, const unsigned *range_bad, const Batch *bt = nullptr, int in = kInPlanes);
// strips by age class (ugsm_kernels_march.hip): share (per mille) of a strip group's rows for the first / second wave of a SIMD; {0, 0} = uniform
extern int march_age_permille[2];
// strip height the marching K-cost picks for a W x H level; host only
int march_strip_rows(int W, int H, int throughput = 0, int pairs = 1);
// The same iteration with the three colour channels on three waves of a workgroup and the epilogue on a fourth (ugsm_kernels_march4.hip): the
// latency form for levels whose launch lasts as long as one strip.  sm.Ws > 0: the level's first iteration, seeded from the coarser field d3.
void launch_cost_march4(hipStream_t st, Img3 L, Img3 R, const float *A3, const float *d3, float *nd3, int W, int H, float thr, int blend, int rows,
                        const unsigned *range_bad, SeedMap sm, const Batch *bt = nullptr);
int march4_strip_rows(int W, int H, int pairs = 1);
// The same iteration for the coarse levels (ugsm_kernels_small.hip): the three channels of a 16 x 12 tile side by side, built for the
// latency of one tile rather than for throughput.
void launch_cost_small(hipStream_t st, Img3 L, Img3 R, const float *A3, const float *d3, float *nd3, int W, int H, float thr, int blend, const Batch *bt = nullptr);

// ---- K-smooth --------------------------------------------------------------------------------
// `passes` Jacobi smoothing passes (+ the 3x3 box when do_box) in one LDS-tiled launch (ugsm_kernels_smooth.hip).
// tile_rows: > 0 = the 112-column tile at this height (1..kSmoothTileRowsMax; smooth_tile_rows picks it); 0 = the tile class by the
// level's size (112 x 36 from 0.5 Mpx, 64 x 32 from 0.26 Mpx, else 32 x 16).
constexpr int kSmoothTileRowsMax = 36;  // (39 rows still fit two workgroups per CU -- 3 x 53 x 128 floats = 81 408 B of LDS -- but the kernel's
                                        // unrolled load / box loops, sized for the tallest tile, then cost every 36-row launch 7.7 % more instructions)
// tile_class (batched launches: the class by what the launch holds, not by one pair's level): 0 = by the level's size, 1 = 32 x 16, 2 = 64 x 32
void launch_smooth_fused(hipStream_t st, const float *s3, float *o3, int W, int H, int passes, int do_box, int tile_rows = 0, const Batch *bt = nullptr,
                         int tile_class = 0);
int smooth_tile_rows(int W, int H, int whole_rounds, int pairs = 1);
extern int smooth_mid_min_pixels;  // (development: UGSM_SMOOTH_MID_MIN)
extern int smooth_lds_extra_bytes; // (development: UGSM_SMOOTH_LDS_EXTRA)
// `passes` (<= 5) Jacobi passes (+ box) for the coarse levels (ugsm_kernels_small.hip): one thread per pixel of an 18 x (rh - 14) tile + halo 7 (rh = 18, 24 or 32)
void launch_smooth_small(hipStream_t st, const float *s3, float *o3, int W, int H, int passes, int do_box, int rh, const Batch *bt = nullptr);

// ---- pyramid, A planes (ugsm_kernels_pyr.hip) ---------------------------------------------------
// range_bad (device word, may be null = unknown): 0 when every pyramid value of the pair passed range_ok (ugsm_exact.hpp),
// which lets K-cost use the range-guarded division; launch_range_scan ORs the check of `count` floats into it.
void launch_range_scan(hipStream_t st, const float *p, size_t count, unsigned *range_bad);
extern int blur_decimate_streaming;  // (development: UGSM_PYR_STREAM)
extern int pyr_base_streaming;       // (development: UGSM_PYR_BASE_STREAM)
extern long long blur_decimate_streaming_min;  // (development: UGSM_PYR_STREAM_MIN)
// zero-padded blur evaluated at the decimation sites
// (range_bad: every level value written is checked as it is produced; may be null)
// stream_min: launches of fewer output pixels keep the LDS-tiled kernel for a factor-2 level too (0 = the streaming kernel k_blur_decimate2 always)
void launch_blur_decimate(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, float sf, unsigned *range_bad, const Batch *bt = nullptr,
                          long long stream_min = 0);
// The part of level 0 a foveated call reads: the fovea window (w x h at (x0, y0), level-0 pixels); w <= 0: everything (full mode).  In a
// batched launch the origin of image b's window is bt->in[b] = (y0 << 32) | x0.
struct PyrWindow {
    int x0, y0, w, h;
};
// ... and the empty window: no tile or strip touches it, so level 0 is not stored at all.  Full-mode calls whose level-0 kernels read the image
// itself (byte_view) build their pyramids with it; levels 1 and 2 come out of the same pass as ever.  (Batched: every origin 0.)
constexpr PyrWindow kPyrNoLevel0{0, 0, 1, 0};
// every image of the launch (rgb, and rgb + bt->img[b]) and the stride 4-byte aligned: what the word-load layouts need (input_layout)
bool input_words_aligned(const uint8_t *rgb, int stride, const Batch *bt);
// fmt: the input format (UGSM_INPUT_*); the four-byte formats take their word-load instances when every image and the stride are 4-byte aligned
void launch_pyr_base(hipStream_t st, const uint8_t *rgb, int stride, int W, int H, float *lvl0, float *lvl1, int W1, int H1, float *lvl2, int W2,
                     int H2, unsigned *range_bad, const Batch *bt = nullptr, PyrWindow win = PyrWindow{0, 0, 0, 0}, int fmt = 0);
// in: kInPlanes -- src is the level's float planes; kInRGB8 -- a byte_view() of the rgb8 image (level 0)
void launch_sqblur_clamp(hipStream_t st, Img3 src, int W, int H, float *dst3, const Batch *bt = nullptr, int in = kInPlanes);

}  // namespace ugsm
