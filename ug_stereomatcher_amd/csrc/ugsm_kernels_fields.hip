// ugsm_kernels_fields.hip -- displacement fields carried between pyramid levels and between fovea stacks.
//
// k_restrict (a level's starting field from a full-resolution prior: the seeded full-mode call), k_prolong (a level's field at full
// resolution in one launch: the coarse half of a full-mode call), k_upsample_paste (one step of hierarchicalDisparity),
// k_upsample_paste_multi (the same step over the stacks of several windows), k_restrict_stack (the starting fields of a warm foveated call
// from a prior stack).  All HBM- or launch-bound; no LDS, no atomics.
// Citations: /root/reference/src/gpu_matcher/<file>:<line> unless a path is given.
#include "ugsm_device.hpp"
#include "ugsm_launch.hpp"

namespace ugsm {

// --------------------------------------------------------------------------------------
// The restriction (ugsm_submit_full_seeded -- no reference counterpart): level s's
// starting field (rm.w x rm.h) from a full-resolution field (rm.W x rm.H, planes dx, dy, conf), read at the sites the image pyramid itself
// samples level s's pixels from.  k = s / 2.  Even s: k steps of the pyramid's sf = 2.0f sampling, tex_index((c + .5f) * 2) -- column x reads
// column ((x + 1) << k) - 1 of level 0; the closed form carries the first k - 1 steps, the last one keeps its tex_index.  Odd s: the same k
// steps down to level 1, c1 = ((x + 1) << k) - 1, then level 1's own site in level 0, tex_index((c1 + .5f) * (float)SCALE).  Rows likewise:
// the source row is one scalar per workgroup.
// Values: dx and dy of an odd level are q = f32((double)v / SCALE), the partner of k_seed's f32(SCALE * (double)v), then q * 2^-k; of an even
// level v * 2^-k (rm.scale = 2^-k, exact in binary32); the confidence is copied.  s = 0: a copy.
// (batched: blockIdx.z = 3 x pair + plane; pair b's full-resolution field at src3 + bt.in[b] bytes)
__device__ __forceinline__ int restrict_site(const int c, const int k, const int odd, const int n)
{
    if (odd) return tex_index(((float)(((c + 1) << k) - 1) + 0.5f) * (float)UGSM_SCALE, n);
    if (k == 0) return c < n ? c : n - 1;
    return tex_index(((float)(((c + 1) << (k - 1)) - 1) + 0.5f) * 2.0f, n);
}
__global__ void k_restrict(const float *__restrict__ src3, RestrictMap rm, float *__restrict__ dst3, Batch bt)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    int plane = blockIdx.z;
    if (bt.n > 1) {
        const int b = plane / 3;
        plane -= 3 * b;
        src3 = shifted(src3, bt.in[b]);
        dst3 = shifted(dst3, bt.out[b]);
    }
    if (ix >= rm.w) return;
    const int sy = restrict_site(iy, rm.k, rm.odd, rm.H);
    const int sx = restrict_site(ix, rm.k, rm.odd, rm.W);
    float v = src3[(size_t)plane * rm.W * rm.H + (size_t)sy * rm.W + sx];
    if (plane < 2) {
        if (rm.odd) v = (float)((double)v / UGSM_SCALE);
        if (rm.k) v = v * rm.scale;
    }
    dst3[(size_t)plane * rm.w * rm.h + (size_t)iy * rm.w + ix] = v;
}
void launch_restrict(hipStream_t st, const float *src3, int W, int H, int level, float *dst3, int w, int h, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    const int k = level / 2;
    const RestrictMap rm{W, H, w, h, k, level & 1, 1.0f / (float)(1 << k)};
    UGSM_LAUNCH(k_restrict, grid2(w, h, 3 * (B.n > 1 ? B.n : 1)), dim3(256), 0, st, src3, rm, dst3, B);
}

// The prolongation (ugsm_submit_full_coarse, ugsm_stage_prolong -- DESIGN.md section 8): the field of level
// e (pm.ws x pm.hs) at full resolution (pm.W x pm.H), pointwise.  By definition e steps of k_seed, P_l = k_seed(P_l+1) for l = e-1 .. 0 with
// no crop; here P_1 .. P_e-1 are never formed: an output pixel walks its column down through the sizes w[1 .. e] -- tex_index(((float)c +
// 0.5f) * sf, w[l]) at every level, whose clamp binds at some levels and not at others, so no closed form --, its row likewise (one site per
// workgroup: blockIdx.y alone decides it), gathers the three planes' values there and multiplies each e times by SCALE in binary64, every
// product rounded to binary32 on its own as the chain rounds it.  e = 0: a copy of a view, like k_copy_view.
// One thread does the three planes of four pixels, in 4 / V pieces of V consecutive pixels (V = pm.vec: 4, 2 or 1 -- what the rows'
// alignment allows, prolong_vec), piece c of a workgroup's 1024 columns at (c * 256 + thread) * V: every store instruction of a wave covers
// consecutive bytes, 16 per lane where V = 4.  The four columns walk down together, a level's size read once for them.  The source is read
// about 2^e times per value, from L2; the launch is bound by the 3 W H floats it writes.  No LDS, no atomics.
// (batched: blockIdx.z = pair; pair b's state at src3 + bt.in[b] bytes, its output at dst3 + bt.out[b] bytes -- moved as pointers, not
// through integers as shifted() does: the accesses stay global ones)
template <int V>
__device__ __forceinline__ void prolong_row(const float *__restrict__ srow, const size_t splane, float *__restrict__ drow, const size_t dplane, const ProlongMap &pm)
{
    struct alignas(4 * V) Vec {
        float v[V];
    };
    const float sf = (float)(1 / UGSM_SCALE);
    int x[4], sx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) sx[k] = x[k] = blockIdx.x * 1024 + ((k / V) * 256 + (int)threadIdx.x) * V + k % V;
    for (int l = 1; l <= pm.e; l++) {
        const int n = pm.w[l];
#pragma unroll
        for (int k = 0; k < 4; k++) sx[k] = tex_index(((float)sx[k] + 0.5f) * sf, n);
    }
#pragma unroll
    for (int c = 0; c < 4 / V; c++) {
        if (x[c * V] >= pm.W) return;  // (pm.W is a multiple of V: a piece lies inside the row or outside it)
        Vec o[3];
#pragma unroll
        for (int j = 0; j < V; j++) {
#pragma unroll
            for (int p = 0; p < 3; p++) {
                float v = srow[p * splane + sx[c * V + j]];
                for (int l = 0; l < pm.e; l++) v = (float)(UGSM_SCALE * (double)v);
                o[p].v[j] = v;
            }
        }
#pragma unroll
        for (int p = 0; p < 3; p++) *reinterpret_cast<Vec *>(drow + p * dplane + x[c * V]) = o[p];
    }
}
__global__ __launch_bounds__(256) void k_prolong(const float *__restrict__ src3, ProlongMap pm, float *__restrict__ dst3, Batch bt)
{
    if (bt.n > 1) {
        src3 = reinterpret_cast<const float *>(reinterpret_cast<const char *>(src3) + bt.in[blockIdx.z]);
        dst3 = reinterpret_cast<float *>(reinterpret_cast<char *>(dst3) + bt.out[blockIdx.z]);
    }
    const float sf = (float)(1 / UGSM_SCALE);
    const int iy = blockIdx.y;
    int sy = iy;
    for (int l = 1; l <= pm.e; l++) sy = tex_index(((float)sy + 0.5f) * sf, pm.h[l]);
    const size_t splane = (size_t)pm.ws * pm.hs, dplane = (size_t)pm.W * pm.H;
    const float *srow = src3 + (size_t)sy * pm.ws;
    float *drow = dst3 + (size_t)iy * pm.W;
    if (pm.vec == 4) prolong_row<4>(srow, splane, drow, dplane, pm);
    else if (pm.vec == 2) prolong_row<2>(srow, splane, drow, dplane, pm);
    else prolong_row<1>(srow, splane, drow, dplane, pm);
}
// the widest store every row of every plane of every pair's output is aligned for: 16 bytes, 8, or 4
static int prolong_vec(const float *dst3, int W, const Batch &B)
{
    for (int v = 4; v > 1; v >>= 1) {
        bool ok = W % v == 0 && reinterpret_cast<uintptr_t>(dst3) % (4 * v) == 0;
        for (int b = 0; ok && b < B.n; b++) ok = B.out[b] % (4 * v) == 0;
        if (ok) return v;
    }
    return 1;
}
bool launch_prolong(hipStream_t st, const float *src3, const int *w, const int *h, int level, float *dst3, const Batch *bt)
{
    Batch one{};
    one.n = 1;
    const Batch &B = bt ? *bt : one;
    if (level < 0 || level >= kProlongMaxLevels || B.n > kMaxBatch || w[0] < 1 || h[0] < 1 || h[0] > 65535) return false;
    ProlongMap pm{};
    pm.W = w[0];
    pm.H = h[0];
    pm.ws = w[level];
    pm.hs = h[level];
    pm.e = level;
    pm.vec = prolong_vec(dst3, w[0], B);
    for (int l = 0; l <= level; l++) {
        if (w[l] < 1 || h[l] < 1) return false;  // (tex_index clamps to n - 1: every read lies inside its level)
        pm.w[l] = w[l];
        pm.h[l] = h[l];
    }
    UGSM_LAUNCH(k_prolong, dim3((w[0] + 1023) / 1024, h[0], B.n > 1 ? B.n : 1), dim3(256), 0, st, src3, pm, dst3, B);
    return true;
}

// =========================================================================================
// one step of hierarchicalDisparity (MatchGPULib.cpp:2643-2683) -- upsample the coarser
// full-frame field by partsubsampleDispKernel (MatchLib.cu:435-462: dst = s * src[tex((x+.5)/s), tex((y+.5)/s)],
// every channel scaled, confidence included) and paste the finer level's fovea at its crop origin, fused: a
// pasted pixel never computes the upsample it would overwrite.  HBM-bound (12 B written per pixel).
// =========================================================================================
__global__ __launch_bounds__(256) void k_upsample_paste(const float *__restrict__ src3, int W, int H, float *__restrict__ dst3, int W2, int H2,
                                                        const float *__restrict__ fovH_, const float *__restrict__ fovV_, const float *__restrict__ fovC_,
                                                        int fovW, int fovH, int org_x, int org_y)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    if (ix >= W2) return;
    const float s = (float)1.41421356;
    const size_t n = (size_t)W * H, n2 = (size_t)W2 * H2, at2 = (size_t)iy * W2 + ix;
    const int fx = ix - org_x, fy = iy - org_y;
    if (fx >= 0 && fx < fovW && fy >= 0 && fy < fovH) {
        const size_t fa = (size_t)fy * fovW + fx;
        dst3[at2] = fovH_[fa];
        dst3[n2 + at2] = fovV_[fa];
        dst3[2 * n2 + at2] = fovC_[fa];
    } else {
        const size_t at = (size_t)tex_index(((float)iy + 0.5f) / s, H) * W + tex_index(((float)ix + 0.5f) / s, W);
        dst3[at2] = s * src3[at];
        dst3[n2 + at2] = s * src3[n + at];
        dst3[2 * n2 + at2] = s * src3[2 * n + at];
    }
}

void launch_upsample_paste(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, const float *fovH_, const float *fovV_,
                           const float *fovC_, int fovW, int fovH, int org_x, int org_y)
{
    UGSM_LAUNCH(k_upsample_paste, dim3((W2 + 255) / 256, H2), dim3(256), 0, st, src3, W, H, dst3, W2, H2, fovH_, fovV_, fovC_, fovW, fovH,
                       org_x, org_y);
}

// The same step over the stacks of pw.n windows of one pair (ugsm_reconstruct_full_multi; PasteWindows, ugsm_launch.hpp): a pixel inside
// window k takes stack k's value -- the HIGHEST such k where windows overlap, found by a loop over the uniform table -- and a pixel inside
// none computes the upsample.  fov0: this level's dx plane in stack 0; its dy and conf planes lie fov_plane, 2 fov_plane floats behind.
// pw.n == 1: the kernel above, operation for operation.
__global__ __launch_bounds__(256) void k_upsample_paste_multi(const float *__restrict__ src3, int W, int H, float *__restrict__ dst3, int W2, int H2,
                                                              const float *__restrict__ fov0, size_t fov_plane, int fovW, int fovH, PasteWindows pw)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    if (ix >= W2) return;
    const float s = (float)1.41421356;
    const size_t n = (size_t)W * H, n2 = (size_t)W2 * H2, at2 = (size_t)iy * W2 + ix;
    int k = -1;
    for (int j = 0; j < pw.n; j++) {
        const int fx = ix - pw.org_x[j], fy = iy - pw.org_y[j];
        if (fx >= 0 && fx < fovW && fy >= 0 && fy < fovH) k = j;
    }
    if (k >= 0) {
        const float *const fov = shifted(fov0, pw.stack[k]);
        const size_t fa = (size_t)(iy - pw.org_y[k]) * fovW + (ix - pw.org_x[k]);
        dst3[at2] = fov[fa];
        dst3[n2 + at2] = fov[fov_plane + fa];
        dst3[2 * n2 + at2] = fov[2 * fov_plane + fa];
    } else {
        const size_t at = (size_t)tex_index(((float)iy + 0.5f) / s, H) * W + tex_index(((float)ix + 0.5f) / s, W);
        dst3[at2] = s * src3[at];
        dst3[n2 + at2] = s * src3[n + at];
        dst3[2 * n2 + at2] = s * src3[2 * n + at];
    }
}

void launch_upsample_paste_multi(hipStream_t st, const float *src3, int W, int H, float *dst3, int W2, int H2, const float *fov0, size_t fov_plane,
                                 int fovW, int fovH, const PasteWindows &pw)
{
    UGSM_LAUNCH(k_upsample_paste_multi, dim3((W2 + 255) / 256, H2), dim3(256), 0, st, src3, W, H, dst3, W2, H2, fov0, fov_plane, fovW, fovH, pw);
}

// The starting fields of a warm foveated call (ugsm_submit_foveated_warm -- no reference counterpart, DESIGN.md section 8;
// RestrictStack, ugsm_launch.hpp): one thread per pixel of the fw x fh starting field of fovea level k of entry e, blockIdx.z = e x (F - s) +
// (k - s), all three planes -- they share the descent.  Window pixel (ix, iy) is level-k pixel (ix + nox[k], iy + noy[k]); its level-0 site is
// restrict_site's; from there the rule of the kernels above is walked from level 0 upwards: level l < F-1 holds the value where the site
// lies inside the prior's window of that level, otherwise it is s * (level l + 1 at tex_index((c + .5f) / s)), the very expressions above.
// The walk's level is uniform (the windows' origins and the levels' sizes come from scalar loads); a lane that has found its level stops
// moving, and the wave leaves the loop when every lane has.  The multiplications by s follow, one per level descended, each rounded on its
// own; then the restriction's value transform (k_restrict's).  Nothing is read outside the prior: a window test precedes every
// read of a level below F-1, and tex_index clamps to level F-1's own size.
template <bool kTable>
__global__ __launch_bounds__(256) void k_restrict_stack(const float *__restrict__ prior0, float *__restrict__ stack0, float *__restrict__ work0, RestrictStack rs)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x;
    const int iy = blockIdx.y;
    const int nl = rs.F - rs.s;
    const int e = blockIdx.z / nl, k = rs.s + (int)blockIdx.z - e * nl;
    const RestrictStackRow &row = kTable ? rs.table[e] : rs.rows[e];
    if (ix >= rs.fw) return;
    const float s = (float)1.41421356;
    const int half = k >> 1, odd = k & 1;
    int x = restrict_site(ix + row.nox[k], half, odd, rs.W);
    int y = restrict_site(iy + row.noy[k], half, odd, rs.H);
    const float *const src = shifted(prior0, row.prior);
    const size_t fn = (size_t)rs.fw * rs.fh;
    size_t at, plane;
    int depth = 0;
    if (rs.field) {
        at = (size_t)y * rs.W + x;
        plane = (size_t)rs.W * rs.H;
    } else {
        plane = (size_t)rs.F * fn;
        bool found = false;
        at = 0;
        for (int l = 0; l < rs.F - 1; l++) {
            const int fx = x - row.pox[l], fy = y - row.poy[l];
            if (!found && fx >= 0 && fx < rs.fw && fy >= 0 && fy < rs.fh) {
                found = true;
                depth = l;
                at = (size_t)l * fn + (size_t)fy * rs.fw + fx;
            }
            if (!found) {
                x = tex_index(((float)x + 0.5f) / s, rs.w[l + 1]);
                y = tex_index(((float)y + 0.5f) / s, rs.h[l + 1]);
            }
            if (__ballot(!found) == 0) break;
        }
        if (!found) {
            depth = rs.F - 1;
            at = (size_t)(rs.F - 1) * fn + (size_t)y * rs.fw + x;
        }
    }
    float v0 = src[at], v1 = src[plane + at], v2 = src[2 * plane + at];
    for (int j = 0; j < depth; j++) {
        v0 = s * v0;
        v1 = s * v1;
        v2 = s * v2;
    }
    if (odd) {
        v0 = (float)((double)v0 / UGSM_SCALE);
        v1 = (float)((double)v1 / UGSM_SCALE);
    }
    if (half) {
        const float scale = __int_as_float((127 - half) << 23);  // 2^-half
        v0 = v0 * scale;
        v1 = v1 * scale;
    }
    const size_t o = (size_t)iy * rs.fw + ix;
    if (work0 && k == rs.s) {
        float *const dst = shifted(work0, row.work);
        dst[o] = v0;
        dst[fn + o] = v1;
        dst[2 * fn + o] = v2;
    } else {
        float *const dst = shifted(stack0, row.dst) + (size_t)k * fn;
        const size_t stack_plane = (size_t)rs.F * fn;
        dst[o] = v0;
        dst[stack_plane + o] = v1;
        dst[2 * stack_plane + o] = v2;
    }
}

bool launch_restrict_stack(hipStream_t st, const float *prior0, float *stack0, float *work0, RestrictStack rs, const RestrictStackRow *rows)
{
    if (!rows || rs.n < 1 || rs.n > kMaxBatch || rs.F < 2 || rs.F > kCloudMaxLevels || rs.s < 0 || rs.s >= rs.F) return false;
    if (rs.fw < 1 || rs.fh < 1 || rs.w[rs.F - 1] != rs.fw || rs.h[rs.F - 1] != rs.fh || rs.w[0] != rs.W || rs.h[0] != rs.H) return false;
    if (!rs.table && rs.n > kRestrictStackByValue) return false;
    for (int e = 0; e < rs.n; e++) {
        const RestrictStackRow &r = rows[e];
        for (int k = rs.s; k < rs.F; k++)
            if (r.nox[k] < 0 || r.noy[k] < 0 || r.nox[k] + rs.fw > rs.w[k] || r.noy[k] + rs.fh > rs.h[k]) return false;
        for (int l = 0; !rs.field && l < rs.F - 1; l++)
            if (r.pox[l] < 0 || r.poy[l] < 0 || r.pox[l] + rs.fw > rs.w[l] || r.poy[l] + rs.fh > rs.h[l]) return false;
        if (!rs.table) rs.rows[e] = r;
    }
    const dim3 grid((rs.fw + 255) / 256, rs.fh, rs.n * (rs.F - rs.s));
    if (rs.table) UGSM_LAUNCH(k_restrict_stack<true>, grid, dim3(256), 0, st, prior0, stack0, work0, rs);
    else UGSM_LAUNCH(k_restrict_stack<false>, grid, dim3(256), 0, st, prior0, stack0, work0, rs);
    return true;
}

}  // namespace ugsm
