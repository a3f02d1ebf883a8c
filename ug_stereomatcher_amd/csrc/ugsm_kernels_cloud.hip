// ugsm_kernels_cloud.hip -- SURVEY 8f row f-1: triangulation of a match into coloured point clouds.
//
// k_cloud / k_cloud_fovea (the coloured cloud and the resized cloud of one field
// or one fovea level), k_cloud_stack (the merged cloud of a whole fovea stack), k_cloud_pairs / k_cloud_stack_pairs (the clouds of the pairs
// of a queue call in one launch), k_cloud_multi (the merged cloud of several windows' stacks).  Every cloud kernel is one tile routine,
// cloud_tile, under a preamble of its own.  A point is ugsm_tri.hpp's, which the plane and depth kernels (ugsm_kernels_depth.hip) share.  HBM-bound.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#include "ugsm_tri.hpp"

namespace ugsm {

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
