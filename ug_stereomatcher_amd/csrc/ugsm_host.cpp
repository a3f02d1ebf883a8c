// ugsm_host.cpp -- everything that touches caller host memory: the host thread team, the images' way up (stage_in), the result planes' way
// into pageable or page-locked memory, the frame of the calls that take images from host memory (host_call), the blocking service calls
// (ugsm_match_*) and the batches from page-locked memory.  What the calls enqueue in between is ugsm_full.cpp and ugsm_fovea.cpp.
#include "ugsm_slot.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <system_error>
#include <thread>

using namespace ugsm;

namespace ugsm {
// A persistent team of host threads for the service path's page touching and staging copies (the first version
// created ~29 std::threads per call; a failed creation -- EAGAIN under a thread or cgroup limit -- threw through an extern "C"
// entry point with joinable threads on the stack, i.e. std::terminate in the caller's process).  Workers are created once, on the
// first service call; creation failures are caught and the team simply stays smaller (down to the calling thread alone).
class HostTeam {
public:
    explicit HostTeam(unsigned want)
    {
        for (unsigned t = 1; t < want; t++) {
            try {
                workers_.emplace_back([this, t] { loop(t); });
            } catch (const std::system_error &) {
                break;  // no more threads to be had: run with what there is
            }
        }
    }
    ~HostTeam()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
            gen_++;
        }
        cv_.notify_all();
        for (std::thread &t : workers_) t.join();
    }
    unsigned size() const { return (unsigned)workers_.size() + 1; }
    // f(member, members) on every member; the caller is member 0.  Returns when all are done.  f must not throw.
    void run(const std::function<void(unsigned, unsigned)> &f)
    {
        const unsigned n = size();
        if (n == 1) {
            f(0, 1);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &f;
            pending_ = n - 1;
            gen_++;
        }
        cv_.notify_all();
        f(0, n);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
    }

private:
    void loop(unsigned me)
    {
        unsigned seen = 0;
        for (;;) {
            const std::function<void(unsigned, unsigned)> *job;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                job = job_;
            }
            if (job) (*job)(me, size());
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned, unsigned)> *job_ = nullptr;
    unsigned gen_ = 0, pending_ = 0;
    bool stop_ = false;
};

}  // namespace ugsm

ugsm_ctx::ugsm_ctx() = default;
ugsm_ctx::~ugsm_ctx() = default;

namespace ugsm {

int stage_in(ugsm_ctx *ctx, Slot &s, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride)
{
    if (!rgbL || !rgbR || W < 1 || H < 1) return UGSM_ERR_BAD_ARG;
    UCHK(input_status(ctx, W, stride, rgbL, rgbR));
    const size_t bytes = (size_t)stride * H;
    UCHK(s.rgb_cap.grow(ctx, bytes, {&s.rgbL, &s.rgbR}));
    HIPCHK(ctx, hipMemcpyAsync(s.rgbL, rgbL, bytes, hipMemcpyHostToDevice, s.st));
    // the right image goes up on the side stream, where its pyramid is built: the transfer (0.9 ms at 16 MP) then runs under the
    // left pyramid instead of in front of it.  The side stream first waits for what the slot did before.
    if (s.alone && s.st2 && ctx->cfg.kernel_path != 1 && ctx->cfg.profile_events == 0 && ctx->two_streams) {  // (single pairs: as side_stream_ok)
        HIPCHK(ctx, hipEventRecord(s.ev_in, s.st));
        s.forked = true;
        HIPCHK(ctx, hipStreamWaitEvent(s.st2, s.ev_in, 0));
        HIPCHK(ctx, hipMemcpyAsync(s.rgbR, rgbR, bytes, hipMemcpyHostToDevice, s.st2));
    } else {
        HIPCHK(ctx, hipMemcpyAsync(s.rgbR, rgbR, bytes, hipMemcpyHostToDevice, s.st));
    }
    return UGSM_OK;
}

namespace {

// Result planes into caller memory.  Page-locked destinations (ugsm_host_alloc, or memory the caller registered) take the
// device-to-host copies directly.  Pageable ones go through a page-locked staging buffer and a team of host threads: the
// reference node allocates fresh result planes for every call (UG_GPU_matcher.cpp:414-418), and the first touch of 193 MB of
// fresh pages by the single copy thread of a pageable hipMemcpy costs more than the whole match (30.7 ms against 16.6 ms per
// 16 MP pair); spread over the team, and with plane k+1's transfer running under plane k's copy, it costs ~2 ms.
bool is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary malloc'd pointer is "invalid value" to the runtime: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// The context's host team (UGSM_COPY_THREADS members, default min(8, hardware threads); 1 = the calling thread only).  Never throws.
HostTeam *host_team(ugsm_ctx *ctx)
{
    if (!ctx->team) {
        const char *e = getenv("UGSM_COPY_THREADS");
        unsigned n = e ? (unsigned)atoi(e) : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
        n = std::min(std::max(1u, n), 64u);
        try {
            ctx->team.reset(new HostTeam(n));
        } catch (...) {  // (allocation failure of the team object itself)
            return nullptr;
        }
    }
    return ctx->team.get();
}

constexpr size_t kTeamMinBytes = 1u << 22;  // below 4 MB a single memcpy / page walk is faster than waking the team

void team_copy(ugsm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    HostTeam *team = bytes >= kTeamMinBytes ? host_team(ctx) : nullptr;
    if (!team || team->size() == 1) {
        memcpy(dst, src, bytes);
        return;
    }
    team->run([=](unsigned t, unsigned n) {
        const size_t chunk = ((bytes / n) + 4095) & ~(size_t)4095;
        const size_t off = (size_t)t * chunk;
        if (off < bytes) memcpy((char *)dst + off, (const char *)src + off, std::min(chunk, bytes - off));
    });
}

// First touch of the caller's (possibly fresh) result pages by the host team WHILE the GPU is still matching: every page of
// dst[0..2] gets one byte written (the planes are overwritten in full afterwards), so the page faults are off the critical path.
void prefault_planes(ugsm_ctx *ctx, float *const dst[3], size_t plane_floats)
{
    const size_t pb = plane_floats * sizeof(float);
    if (pb < kTeamMinBytes) return;  // (a small call: the copy itself touches the pages)
    if (is_pinned(dst[0]) && is_pinned(dst[1]) && is_pinned(dst[2])) return;
    auto touch = [=](unsigned t, unsigned n) {
        for (int k = 0; k < 3; k++) {
            volatile char *p = (volatile char *)dst[k];
            const size_t lo = pb * t / n, hi = pb * (t + 1) / n;
            for (size_t o = (lo + 4095) & ~(size_t)4095; o < hi; o += 4096) p[o] = 0;
            if (t == 0 && pb) p[0] = 0;
        }
    };
    HostTeam *team = host_team(ctx);
    if (team) team->run(touch);
    else touch(0, 1);
}

int copy_out_planes(ugsm_ctx *ctx, Slot &s, const float *d_src, size_t plane_floats, float *const dst[3])
{
    const size_t pb = plane_floats * sizeof(float);
    if (is_pinned(dst[0]) && is_pinned(dst[1]) && is_pinned(dst[2])) {
        for (int k = 0; k < 3; k++) HIPCHK(ctx, hipMemcpyAsync(dst[k], d_src + k * plane_floats, pb, hipMemcpyDeviceToHost, s.st));
        return UGSM_OK;
    }
    UCHK(s.hpin.grow(ctx, 3 * plane_floats));
    // Every plane in PIECES: a piece's copy into the caller's pages runs under the next piece's transfer, so what is left exposed behind
    // the last transfer is one piece's copy, not one plane's (a quarter plane at 16 MP: 0.25 ms instead of 1 ms).
    const int pieces = pb >= 4 * kTeamMinBytes ? 4 : 1;
    const size_t pf = ((plane_floats + pieces - 1) / pieces + 1023) & ~(size_t)1023;  // floats per piece (4 KiB multiples)
    auto piece = [&](int i, size_t &off, size_t &len) {
        const int k = i / pieces, c = i - k * pieces;
        const size_t lo = std::min((size_t)c * pf, plane_floats), hi = std::min(lo + pf, plane_floats);
        off = (size_t)k * plane_floats + lo;
        len = hi - lo;
        return k;
    };
    for (int i = 0; i < 3 * pieces; i++) {
        size_t off, len;
        piece(i, off, len);
        if (!s.out_ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&s.out_ev[i], hipEventDisableTiming));
        if (len) HIPCHK(ctx, hipMemcpyAsync(s.hpin + off, d_src + off, len * sizeof(float), hipMemcpyDeviceToHost, s.st));
        HIPCHK(ctx, hipEventRecord(s.out_ev[i], s.st));
    }
    for (int i = 0; i < 3 * pieces; i++) {
        size_t off, len;
        const int k = piece(i, off, len);
        HIPCHK(ctx, hipEventSynchronize(s.out_ev[i]));
        if (len) team_copy(ctx, (char *)dst[k] + (off - (size_t)k * plane_floats) * sizeof(float), s.hpin + off, len * sizeof(float));
    }
    return UGSM_OK;
}

// One buffer of any size into caller memory of either kind (the depth image; a single plane): a page-locked destination takes the copy
// directly, a pageable one takes it through the front of the slot's page-locked staging and the host team -- whatever went through the
// staging before has been copied out by then (copy_out_planes and this function return with their pageable copies done).
int copy_out_bytes(ugsm_ctx *ctx, Slot &s, const void *d_src, size_t bytes, void *dst)
{
    if (is_pinned(dst)) {
        HIPCHK(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, s.st));
        return UGSM_OK;
    }
    UCHK(s.hpin.grow(ctx, (bytes + 3) / 4));
    if (!s.out_ev[0]) HIPCHK(ctx, hipEventCreateWithFlags(&s.out_ev[0], hipEventDisableTiming));
    HIPCHK(ctx, hipMemcpyAsync(s.hpin, d_src, bytes, hipMemcpyDeviceToHost, s.st));
    HIPCHK(ctx, hipEventRecord(s.out_ev[0], s.st));
    HIPCHK(ctx, hipEventSynchronize(s.out_ev[0]));
    team_copy(ctx, dst, s.hpin, bytes);
    return UGSM_OK;
}

// The counterpart of copy_out_planes for what a call reads besides its images (a prior, a state, a prior stack): three host planes of any kind
// up into d_dst, on the slot's stream.
int upload_planes(ugsm_ctx *ctx, Slot &s, float *d_dst, size_t plane_floats, const float *const src[3])
{
    for (int c = 0; c < 3; c++) HIPCHK(ctx, hipMemcpyAsync(d_dst + c * plane_floats, src[c], plane_floats * sizeof(float), hipMemcpyHostToDevice, s.st));
    return UGSM_OK;
}

// a device stack's H, V and C planes (stackn floats each) down into three host buffers, on the slot's stream
int download_stack(ugsm_ctx *ctx, Slot &s, const float *d_stack, size_t stackn, float *stackH, float *stackV, float *stackC)
{
    float *const dst[3] = {stackH, stackV, stackC};
    for (int c = 0; c < 3; c++) HIPCHK(ctx, hipMemcpyAsync(dst[c], d_stack + c * stackn, stackn * sizeof(float), hipMemcpyDeviceToHost, s.st));
    return UGSM_OK;
}

// what the non-blocking host-memory calls answer to a buffer that is not page-locked
int not_pinned(ugsm_ctx *ctx, const char *entry)
{
    ctx->err = std::string(entry) + ": every host buffer must be page-locked (ugsm_host_alloc, hipHostMalloc or hipHostRegister)";
    return UGSM_ERR_BAD_ARG;
}

// A blocking entry point that failed part-way: whatever it did enqueue -- uploads that read the caller's images, on the slot's stream or on
// the side stream -- has drained before the caller hears of the failure.  "When the call returns the buffers are the caller's again"
// holds for a failed call too (the reference exit()s instead, MatchGPULib.cpp passim).
int drained(ugsm_ctx *ctx, int slot, int st)
{
    if (st == UGSM_OK || !ctx || slot < 0 || slot >= (int)ctx->slots.size()) return st;
    const std::string why = ctx->err;
    (void)ugsm_wait(ctx, slot);
    ctx->err = why;
    return st;
}

// The frame of every call that takes one pair's images from host memory, on a slot.  `sync`: the reference's call -- it returns when the results
// are in place, in pageable or page-locked memory, and a failure part-way is drained --; otherwise everything is only enqueued and every buffer
// must be page-locked.  The slot, the device, then what the call brings:
//   check(slot, hout): the call's own refusals, in the call's own order, and `hout`, the floats of the slot's result staging it needs; a call
//       that must hear UGSM_ERR_NOMEM before anything is enqueued grows its buffers, the staging included, here;
//   the images go up into slot.rgbL / rgbR (stage_in), the result staging grows;
//   match(slot): the uploads of what the call reads besides the images, and the match, into the staging it carves itself;
//   down(slot): the results into the caller's memory;
// and the wait, or the completion mark.
template <class Check, class Match, class Down>
int host_call(ugsm_ctx *ctx, int slot, bool sync, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, Check &&check, Match &&match,
              Down &&down)
{
    auto enqueue = [&]() -> int {
        Slot *s;
        UCHK(get_slot(ctx, slot, &s));
        HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
        size_t hout = 0;
        UCHK(check(*s, hout));
        UCHK(stage_in(ctx, *s, rgbL, rgbR, W, H, stride));
        UCHK(s->hout.grow(ctx, hout));
        UCHK(match(*s));
        UCHK(down(*s));
        if (!sync) return mark_done(ctx, *s);
        s->forked = false;  // (enqueued whole, as mark_done)
        return ugsm_wait(ctx, slot);
    };
    return sync ? drained(ctx, slot, enqueue()) : enqueue();
}
// ... of a blocking call on slot 0 whose entry point has made every refusal (ugsm_seeded.cpp, ugsm_coarse.cpp, ugsm_fovea_seeded.cpp)
template <class Match, class Down>
int host_call(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, size_t hout_floats, Match &&match, Down &&down)
{
    auto size = [&](Slot &, size_t &hout) -> int {
        hout = hout_floats;
        return UGSM_OK;
    };
    return host_call(ctx, 0, true, rgbL, rgbR, W, H, stride, size, match, down);
}

}  // namespace

// The seeded service call (ugsm_match_full_seeded) on slot 0: images and prior up -- the prior's planes into the slot's result staging, where
// the call then writes in place: the restriction reads before level 0 writes --, the match, the planes into caller memory of any kind.
int seeded_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const float *const prior[3], int start_level,
                 float *const disp[3])
{
    const size_t n = (size_t)W * H;
    auto match = [&](Slot &s) -> int {
        UCHK(upload_planes(ctx, s, s.hout, n, prior));
        const LevelRange r = LevelRange::seeded(start_level, &s.hout.p);
        return enqueue_match_full(ctx, s, 0, 1, &s.rgbL.p, &s.rgbR.p, W, H, stride, &s.hout.p, &r);
    };
    return host_call(ctx, rgbL, rgbR, W, H, stride, 3 * n, match, [&](Slot &s) -> int {
        prefault_planes(ctx, disp, n);
        return copy_out_planes(ctx, s, s.hout, n, disp);
    });
}

// The two halves as service calls (ugsm_match_full_coarse, ugsm_match_full_fine) on slot 0.  The slot's result staging holds the
// full-resolution field (the prolongation, or the fine half's result) and, behind it, the state of level e (whose size the entry point has had).
int coarse_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int e, float *const state[3], float *const full[3])
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));  // (holds: the entry point has had level e's size from it)
    const size_t n = (size_t)W * H, ne = (size_t)w[e] * h[e], room = full ? field_room(n) : 0;
    auto match = [&](Slot &s) -> int {
        float *const d_state = s.hout + room, *const d_full = full ? s.hout : nullptr;
        const LevelRange r = LevelRange::coarse(ctx->cfg.levels, e, &d_full);
        return enqueue_match_full(ctx, s, 0, 1, &s.rgbL.p, &s.rgbR.p, W, H, stride, &d_state, &r);
    };
    return host_call(ctx, rgbL, rgbR, W, H, stride, room + 3 * ne, match, [&](Slot &s) -> int {
        if (full) prefault_planes(ctx, full, n);
        UCHK(copy_out_planes(ctx, s, s.hout + room, ne, state));
        return full ? copy_out_planes(ctx, s, s.hout, n, full) : UGSM_OK;
    });
}
int fine_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const float *const state[3], int e, float *const disp[3])
{
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    UCHK(level_dims(W, H, ctx->cfg.levels, w, h));
    const size_t n = (size_t)W * H, ne = (size_t)w[e] * h[e], room = field_room(n);
    auto match = [&](Slot &s) -> int {
        UCHK(upload_planes(ctx, s, s.hout + room, ne, state));
        const float *const d_state = s.hout + room;
        const LevelRange r = LevelRange::fine(e, &d_state);
        return enqueue_match_full(ctx, s, 0, 1, &s.rgbL.p, &s.rgbR.p, W, H, stride, &s.hout.p, &r);
    };
    return host_call(ctx, rgbL, rgbR, W, H, stride, room + 3 * ne, match, [&](Slot &s) -> int {
        prefault_planes(ctx, disp, n);
        return copy_out_planes(ctx, s, s.hout, n, disp);
    });
}

// The warm foveated service call (ugsm_match_foveated_warm) on slot 0: images and the prior stack's three planes up, the match into a second
// stack beside it in the slot's result staging (the call is not in place: [prior stack][stack]), that stack's planes down.
int fovea_warm_match(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y, const float *const prior[3],
                     int prior_off_x, int prior_off_y, int start_level, float *const stack[3])
{
    FoveaRoom room;
    UCHK(fovea_room(ctx, W, H, FoveaCall::Warm, 1, room));
    const size_t at_prior = room.part(room.stack), at_stack = room.part(room.stack);
    auto match = [&](Slot &s) -> int {
        UCHK(upload_planes(ctx, s, s.hout + at_prior, room.plane, prior));
        const float *const d_prior = s.hout + at_prior;
        float *const d_stack = s.hout + at_stack;
        return enqueue_foveated(ctx, s, 0, &s.rgbL.p, &s.rgbR.p, W, H, stride,
                                FoveaCall::warm(1, &off_x, &off_y, &d_prior, &prior_off_x, &prior_off_y, false, start_level, &d_stack));
    };
    return host_call(ctx, rgbL, rgbR, W, H, stride, room.total, match,
                     [&](Slot &s) -> int { return download_stack(ctx, s, s.hout + at_stack, room.plane, stack[0], stack[1], stack[2]); });
}

void ctx_host_copy(ugsm_ctx *ctx, void *dst, const void *src, size_t bytes) { team_copy(ctx, dst, src, bytes); }
bool host_pinned(const void *p) { return is_pinned(p); }
}  // namespace ugsm

extern "C" {

// The service call on a slot: upload, pyramids, match, results into caller memory (host_call: `sync` = the reference's call).
static int match_full_host(ugsm_ctx *ctx, int slot, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float *dispH, float *dispV,
                           float *dispC, bool sync)
{
    float *const dst[3] = {dispH, dispV, dispC};
    const size_t n = (size_t)W * H;
    auto check = [&](Slot &, size_t &hout) -> int {
        if (!dispH || !dispV || !dispC) return UGSM_ERR_BAD_ARG;
        if (!sync && !(is_pinned(rgbL) && is_pinned(rgbR) && is_pinned(dispH) && is_pinned(dispV) && is_pinned(dispC))) return not_pinned(ctx, "ugsm_submit_full_host");
        hout = 3 * n;
        return UGSM_OK;
    };
    auto match = [&](Slot &s) -> int { return enqueue_match_full(ctx, s, slot, 1, &s.rgbL.p, &s.rgbR.p, W, H, stride, &s.hout.p); };
    return host_call(ctx, slot, sync, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        if (sync) prefault_planes(ctx, dst, n);  // the GPU is busy for the next ~10 ms: touch the caller's result pages meanwhile
        return copy_out_planes(ctx, s, s.hout, n, dst);
    });
}

int ugsm_match_full(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float *dispH,
                    float *dispV, float *dispC)
{
    return match_full_host(ctx, 0, rgbL, rgbR, W, H, stride, dispH, dispV, dispC, true);
}

// The service call with the depth image (REP 118) as its result: ugsm_match_full, then ugsm_depth_image on the same slot from the planes
// in the slot's result staging, the image behind them; the image comes down, and whichever planes are asked for.
int ugsm_match_full_depth(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const double *P1, const double *P2,
                          const ugsm_depth_params *p, void *depth, float *dispH, float *dispV, float *dispC)
{
    float *const dst[3] = {dispH, dispV, dispC};
    const bool all_planes = dispH && dispV && dispC;
    const size_t n = (size_t)W * H, room = field_room(n);
    size_t image_bytes = 0;
    auto check = [&](Slot &, size_t &hout) -> int {
        int dw, dh;
        if (!depth || !P1 || !P2) return UGSM_ERR_BAD_ARG;
        UCHK(depth_params_ok(p, true, W, H, &dw, &dh));
        image_bytes = (size_t)dw * dh * (p->format == UGSM_DEPTH_16U ? 2 : 4);
        hout = room + (image_bytes + 3) / 4;
        return UGSM_OK;
    };
    auto match = [&](Slot &s) -> int {
        UCHK(enqueue_match_full(ctx, s, 0, 1, &s.rgbL.p, &s.rgbR.p, W, H, stride, &s.hout.p));
        return ugsm_depth_image(ctx, 0, s.hout, s.hout + n, s.hout + 2 * n, W, H, P1, P2, p, s.hout + room, nullptr);
    };
    return host_call(ctx, 0, true, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        if (all_planes) {
            prefault_planes(ctx, dst, n);
            UCHK(copy_out_planes(ctx, s, s.hout, n, dst));
        } else {
            for (int k = 0; k < 3; k++)
                if (dst[k]) UCHK(copy_out_bytes(ctx, s, s.hout + k * n, n * sizeof(float), dst[k]));
        }
        return copy_out_bytes(ctx, s, s.hout + room, image_bytes, depth);
    });
}

int ugsm_submit_full_host(ugsm_ctx *ctx, int slot, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float *dispH,
                          float *dispV, float *dispC)
{
    return match_full_host(ctx, slot, rgbL, rgbR, W, H, stride, dispH, dispV, dispC, false);
}

// The checked service call on slot 0: upload, both directions in lockstep, the check, the forward planes (and the backward ones where asked
// for) into caller memory of any kind.  Its buffers, the result staging included, grow before the images go up.
int ugsm_match_full_checked(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float *dispH, float *dispV,
                            float *dispC, float *backH, float *backV, float *backC, float tau)
{
    float *const dst[3] = {dispH, dispV, dispC}, *const bdst[3] = {backH, backV, backC};
    const bool back = backH || backV || backC;
    const size_t n = (size_t)W * H, room = field_room(n);
    auto check = [&](Slot &s, size_t &hout) -> int {
        if (!rgbL || !rgbR || !dispH || !dispV || !dispC) return UGSM_ERR_BAD_ARG;
        if (back && !(backH && backV && backC)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "backH, backV and backC: all three or none");
        UCHK(full_checked_check(ctx, 1, W, H, stride, tau));
        UCHK(full_checked_bufs(ctx, s, 1, back ? 0 : 1, W, H));
        hout = (back ? 2 : 1) * room;
        return s.hout.grow(ctx, hout);
    };
    auto match = [&](Slot &s) -> int {
        float *const d_fwd = s.hout, *const d_bwd = back ? s.hout + room : nullptr;
        return enqueue_full_checked(ctx, s, 0, 1, &s.rgbL.p, &s.rgbR.p, W, H, stride, &d_fwd, back ? &d_bwd : nullptr, tau);
    };
    return host_call(ctx, 0, true, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        prefault_planes(ctx, dst, n);
        if (back) prefault_planes(ctx, bdst, n);
        UCHK(copy_out_planes(ctx, s, s.hout, n, dst));
        return back ? copy_out_planes(ctx, s, s.hout + room, n, bdst) : UGSM_OK;
    });
}

// One foveated pair from host memory.  Behind the state in the slot's result staging: [stack][pyrL][pyrR], the pyramid stacks where they are
// asked for.
static int match_foveated_host(ugsm_ctx *ctx, int slot, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                               float *stackH, float *stackV, float *stackC, float *pyrL, float *pyrR, bool sync)
{
    FoveaRoom room;
    size_t at_stack = 0, at_pl = 0, at_pr = 0;
    float *d_stack = nullptr, *d_pl = nullptr, *d_pr = nullptr;
    auto check = [&](Slot &, size_t &hout) -> int {
        if (!stackH || !stackV || !stackC || ctx->cfg.fovea_levels < 2) return UGSM_ERR_BAD_ARG;
        if (!sync && !(is_pinned(rgbL) && is_pinned(rgbR) && is_pinned(stackH) && is_pinned(stackV) && is_pinned(stackC) && (!pyrL || is_pinned(pyrL)) &&
                       (!pyrR || is_pinned(pyrR))))
            return not_pinned(ctx, "ugsm_submit_foveated_host");
        UCHK(fovea_room(ctx, W, H, FoveaCall::Pairs, 1, room));
        at_stack = room.part(room.stack);
        if (pyrL) at_pl = room.part(room.stack);
        if (pyrR) at_pr = room.part(room.stack);
        hout = room.total;
        return UGSM_OK;
    };
    auto match = [&](Slot &s) -> int {
        d_stack = s.hout + at_stack;
        d_pl = pyrL ? s.hout + at_pl : nullptr;
        d_pr = pyrR ? s.hout + at_pr : nullptr;
        return enqueue_foveated(ctx, s, slot, &s.rgbL.p, &s.rgbR.p, W, H, stride, FoveaCall::pairs(1, &off_x, &off_y, &d_stack, &d_pl, &d_pr));
    };
    return host_call(ctx, slot, sync, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        UCHK(download_stack(ctx, s, d_stack, room.plane, stackH, stackV, stackC));
        if (pyrL) HIPCHK(ctx, hipMemcpyAsync(pyrL, d_pl, room.stack * sizeof(float), hipMemcpyDeviceToHost, s.st));
        if (pyrR) HIPCHK(ctx, hipMemcpyAsync(pyrR, d_pr, room.stack * sizeof(float), hipMemcpyDeviceToHost, s.st));
        return UGSM_OK;
    });
}

int ugsm_match_foveated(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x,
                        int off_y, float *stackH, float *stackV, float *stackC, float *pyrL, float *pyrR)
{
    return match_foveated_host(ctx, 0, rgbL, rgbR, W, H, stride, off_x, off_y, stackH, stackV, stackC, pyrL, pyrR, true);
}

// The foveated service call with the whole frame's depth image (REP 118) as its result: ugsm_match_foveated, then
// ugsm_depth_image_fovea_full on the same slot from the stack in the slot's result staging, the image behind it; the image comes down, and
// whichever stack planes are asked for.  The sibling of ugsm_match_full_depth.
int ugsm_match_foveated_depth(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                              const double *P1, const double *P2, const ugsm_depth_params *p, void *depth, float *stackH, float *stackV, float *stackC)
{
    float *const dst[3] = {stackH, stackV, stackC};
    FoveaRoom room;
    size_t at_stack = 0, at_image = 0, image_bytes = 0;
    auto check = [&](Slot &, size_t &hout) -> int {
        int dw, dh;
        if (!depth || !P1 || !P2 || ctx->cfg.fovea_levels < 2) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_match_foveated_depth: a null pointer, or fovea_levels < 2");
        if (depth_params_ok(p, true, W, H, &dw, &dh) != UGSM_OK) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_match_foveated_depth: the depth parameters");
        image_bytes = (size_t)dw * dh * (p->format == UGSM_DEPTH_16U ? 2 : 4);
        UCHK(fovea_room(ctx, W, H, FoveaCall::Pairs, 1, room));
        at_stack = room.part(room.stack);
        at_image = room.part((image_bytes + 3) / 4);
        hout = room.total;
        return UGSM_OK;
    };
    auto match = [&](Slot &s) -> int {
        float *d_stack = s.hout + at_stack, *d_none = nullptr;
        UCHK(enqueue_foveated(ctx, s, 0, &s.rgbL.p, &s.rgbR.p, W, H, stride, FoveaCall::pairs(1, &off_x, &off_y, &d_stack, &d_none, &d_none)));
        return ugsm_depth_image_fovea_full(ctx, 0, d_stack, d_stack + room.plane, d_stack + 2 * room.plane, W, H, off_x, off_y, P1, P2, p,
                                           s.hout + at_image, nullptr);
    };
    return host_call(ctx, 0, true, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        for (int k = 0; k < 3; k++)
            if (dst[k]) UCHK(copy_out_bytes(ctx, s, s.hout + at_stack + k * room.plane, room.plane * sizeof(float), dst[k]));
        return copy_out_bytes(ctx, s, s.hout + at_image, image_bytes, depth);
    });
}

int ugsm_submit_foveated_host(ugsm_ctx *ctx, int slot, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x,
                              int off_y, float *stackH, float *stackV, float *stackC, float *pyrL, float *pyrR)
{
    return match_foveated_host(ctx, slot, rgbL, rgbR, W, H, stride, off_x, off_y, stackH, stackV, stackC, pyrL, pyrR, false);
}

// n windows of one pair from host memory, on slot 0 (tau: null = the plain call, else the checked one's threshold).  Behind the state in the
// slot's result staging: the n stacks; the call's buffers, the staging included, grow before the images go up.
static int match_foveated_multi_host(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int n, const int *off_x,
                                     const int *off_y, float *const *stackH, float *const *stackV, float *const *stackC, const float *tau)
{
    FoveaRoom room;
    float *d_stack[UGSM_MAX_BATCH];
    const FoveaCall plain = FoveaCall::windows(n, off_x, off_y, d_stack), call = tau ? plain.checked(*tau) : plain;
    auto check = [&](Slot &s, size_t &hout) -> int {
        if (!rgbL || !rgbR || !stackH || !stackV || !stackC) return UGSM_ERR_BAD_ARG;
        for (int k = 0; k < n && k < UGSM_MAX_BATCH; k++)
            if (!stackH[k] || !stackV[k] || !stackC[k]) return UGSM_ERR_BAD_ARG;
        UCHK(multi_check(ctx, n, W, H, stride, tau));
        UCHK(fovea_room(ctx, W, H, call.kind, n, room));
        const size_t at_stacks = room.part(n * room.stack);
        UCHK(fovea_grow(ctx, s, W, H, call, room));
        for (int k = 0; k < n; k++) d_stack[k] = s.hout + at_stacks + k * room.stack;
        hout = room.total;
        return UGSM_OK;
    };
    auto match = [&](Slot &s) -> int { return enqueue_foveated(ctx, s, 0, &s.rgbL.p, &s.rgbR.p, W, H, stride, call); };
    return host_call(ctx, 0, true, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        for (int k = 0; k < n; k++) UCHK(download_stack(ctx, s, d_stack[k], room.plane, stackH[k], stackV[k], stackC[k]));
        return UGSM_OK;
    });
}

int ugsm_match_foveated_multi(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int n, const int *off_x,
                              const int *off_y, float *const *stackH, float *const *stackV, float *const *stackC)
{
    return match_foveated_multi_host(ctx, rgbL, rgbR, W, H, stride, n, off_x, off_y, stackH, stackV, stackC, nullptr);
}

int ugsm_match_foveated_multi_checked(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int n, const int *off_x,
                                      const int *off_y, float *const *stackH, float *const *stackV, float *const *stackC, float tau)
{
    return match_foveated_multi_host(ctx, rgbL, rgbR, W, H, stride, n, off_x, off_y, stackH, stackV, stackC, &tau);
}

// match(L, R, fov == 1), MatchGPULib.cpp:354-360: foveated matching, then hierarchicalDisparity on the stacks.  Behind the state in the slot's
// result staging: [stack][full field]
int ugsm_match_foveated_full(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                             float *outH, float *outV, float *outC)
{
    float *const dst[3] = {outH, outV, outC};
    const size_t n = (size_t)W * H;
    FoveaRoom room;
    size_t at_stack = 0, at_full = 0;
    auto check = [&](Slot &, size_t &hout) -> int {
        if (!outH || !outV || !outC || ctx->cfg.fovea_levels < 2) return UGSM_ERR_BAD_ARG;
        UCHK(fovea_room(ctx, W, H, FoveaCall::Pairs, 1, room));
        at_stack = room.part(room.stack);
        at_full = room.part(3 * n);
        hout = room.total;
        return UGSM_OK;
    };
    auto match = [&](Slot &s) -> int {
        float *d_stack = s.hout + at_stack;
        UCHK(enqueue_foveated(ctx, s, 0, &s.rgbL.p, &s.rgbR.p, W, H, stride, FoveaCall::pairs(1, &off_x, &off_y, &d_stack)));
        return ugsm_reconstruct_full(ctx, 0, d_stack, d_stack + room.plane, d_stack + 2 * room.plane, W, H, off_x, off_y, s.hout + at_full);
    };
    return host_call(ctx, 0, true, rgbL, rgbR, W, H, stride, check, match, [&](Slot &s) -> int {
        prefault_planes(ctx, dst, n);
        return copy_out_planes(ctx, s, s.hout + at_full, n, dst);
    });
}

// ---- batches from page-locked host memory (round 4): the uploads of all pairs, ONE batched match, the downloads of all pairs, enqueued on
// the slot's stream.  The images are staged in the slot (pair b at rgbL / rgbR + b * image bytes), the results in hout.
static bool all_pinned(const void *const *p, int n)
{
    for (int b = 0; b < n; b++)
        if (!p[b] || !is_pinned(p[b])) return false;
    return true;
}
// what both calls refuse behind their null arrays: an image or a result plane, of any pair, that is null or not page-locked
static int batch_pinned(ugsm_ctx *ctx, const char *entry, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR, float *const *outH,
                        float *const *outV, float *const *outC)
{
    for (const void *const *p : {(const void *const *)rgbL, (const void *const *)rgbR, (const void *const *)outH, (const void *const *)outV, (const void *const *)outC})
        if (!all_pinned(p, n)) return not_pinned(ctx, entry);
    return UGSM_OK;
}
static int stage_in_batch(ugsm_ctx *ctx, Slot &s, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR, int W, int H, int stride,
                          const uint8_t **dL, const uint8_t **dR)
{
    if (W < 1 || H < 1) return UGSM_ERR_BAD_ARG;
    for (int b = 0; b < n; b++) UCHK(input_status(ctx, W, stride, rgbL[b], rgbR[b]));
    const size_t bytes = ((size_t)stride * H + 255) & ~(size_t)255;
    UCHK(s.rgb_cap.grow(ctx, bytes * n, {&s.rgbL, &s.rgbR}));
    for (int b = 0; b < n; b++) {
        dL[b] = s.rgbL + b * bytes;
        dR[b] = s.rgbR + b * bytes;
        HIPCHK(ctx, hipMemcpyAsync(s.rgbL + b * bytes, rgbL[b], (size_t)stride * H, hipMemcpyHostToDevice, s.st));
        HIPCHK(ctx, hipMemcpyAsync(s.rgbR + b * bytes, rgbR[b], (size_t)stride * H, hipMemcpyHostToDevice, s.st));
    }
    return UGSM_OK;
}

int ugsm_submit_full_batch_host(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR, int W, int H, int stride,
                                float *const *dispH, float *const *dispV, float *const *dispC)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (n < 1 || n > UGSM_MAX_BATCH || !rgbL || !rgbR || !dispH || !dispV || !dispC) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(batch_pinned(ctx, "ugsm_submit_full_batch_host", n, rgbL, rgbR, dispH, dispV, dispC));
    if (n == 1 || batch_runs_pair_by_pair(ctx)) {
        for (int b = 0; b < n; b++) UCHK(match_full_host(ctx, slot, rgbL[b], rgbR[b], W, H, stride, dispH[b], dispV[b], dispC[b], false));
        return UGSM_OK;
    }
    const uint8_t *dL[UGSM_MAX_BATCH], *dR[UGSM_MAX_BATCH];
    UCHK(stage_in_batch(ctx, *s, n, rgbL, rgbR, W, H, stride, dL, dR));
    const size_t px = (size_t)W * H, per = field_room(px);
    UCHK(s->hout.grow(ctx, per * n));
    float *out[UGSM_MAX_BATCH];
    for (int b = 0; b < n; b++) out[b] = s->hout + b * per;
    UCHK(enqueue_match_full(ctx, *s, slot, n, dL, dR, W, H, stride, out));
    for (int b = 0; b < n; b++) {
        float *const dst[3] = {dispH[b], dispV[b], dispC[b]};
        UCHK(copy_out_planes(ctx, *s, out[b], px, dst));  // (page-locked destinations: three asynchronous copies)
    }
    return mark_done(ctx, *s);
}

// The checked call from page-locked memory: the uploads of all pairs, both directions in ONE lockstep match (enqueue_full_checked, a lone pair
// too: the call has no pair-by-pair form), the downloads -- every pair's checked forward planes, and the backward ones of the pairs that ask.
// The slot's result staging: [n forward fields][the back fields that are taken], field_room floats each.  Every buffer, the staging included,
// grows before anything is enqueued.
int ugsm_submit_full_checked_host(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR, int W, int H, int stride,
                                  float *const *dispH, float *const *dispV, float *const *dispC, float *const *backH, float *const *backV,
                                  float *const *backC, float tau)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (!rgbL || !rgbR || !dispH || !dispV || !dispC) return UGSM_ERR_BAD_ARG;
    UCHK(full_checked_check(ctx, n, W, H, stride, tau));
    const bool backs = backH || backV || backC;
    if (backs && !(backH && backV && backC)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "backH, backV and backC: all three arrays or none");
    bool takes[UGSM_MAX_BATCH];
    int taken = 0;
    for (int b = 0; b < n; b++) {
        const int given = backs ? (backH[b] != nullptr) + (backV[b] != nullptr) + (backC[b] != nullptr) : 0;
        if (given != 0 && given != 3) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "backH, backV and backC of a pair: all three or none");
        takes[b] = given == 3;
        taken += takes[b];
    }
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(batch_pinned(ctx, "ugsm_submit_full_checked_host", n, rgbL, rgbR, dispH, dispV, dispC));
    for (int b = 0; b < n; b++)
        if (takes[b] && !(is_pinned(backH[b]) && is_pinned(backV[b]) && is_pinned(backC[b]))) return not_pinned(ctx, "ugsm_submit_full_checked_host");
    const size_t px = (size_t)W * H, per = field_room(px);
    UCHK(full_checked_bufs(ctx, *s, n, n - taken, W, H));
    UCHK(s->hout.grow(ctx, per * (n + taken)));
    const uint8_t *dL[UGSM_MAX_BATCH], *dR[UGSM_MAX_BATCH];
    UCHK(stage_in_batch(ctx, *s, n, rgbL, rgbR, W, H, stride, dL, dR));
    float *out[UGSM_MAX_BATCH], *back[UGSM_MAX_BATCH];
    for (int b = 0, k = 0; b < n; b++) {
        out[b] = s->hout + b * per;
        back[b] = takes[b] ? s->hout + (n + k++) * per : nullptr;
    }
    UCHK(enqueue_full_checked(ctx, *s, slot, n, dL, dR, W, H, stride, out, taken ? back : nullptr, tau));
    for (int b = 0; b < n; b++) {
        float *const dst[3] = {dispH[b], dispV[b], dispC[b]};
        UCHK(copy_out_planes(ctx, *s, out[b], px, dst));  // (page-locked destinations: three asynchronous copies)
        if (!takes[b]) continue;
        float *const bdst[3] = {backH[b], backV[b], backC[b]};
        UCHK(copy_out_planes(ctx, *s, back[b], px, bdst));
    }
    return mark_done(ctx, *s);
}

int ugsm_submit_foveated_batch_host(ugsm_ctx *ctx, int slot, int n, const uint8_t *const *rgbL, const uint8_t *const *rgbR, int W, int H, int stride,
                                    const int *off_x, const int *off_y, float *const *stackH, float *const *stackV, float *const *stackC)
{
    Slot *s;
    UCHK(get_slot(ctx, slot, &s));
    if (n < 1 || n > UGSM_MAX_BATCH || !rgbL || !rgbR || !stackH || !stackV || !stackC) return UGSM_ERR_BAD_ARG;
    const int F = ctx->cfg.fovea_levels;
    if (F < 2) return UGSM_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->cfg.device));
    UCHK(batch_pinned(ctx, "ugsm_submit_foveated_batch_host", n, rgbL, rgbR, stackH, stackV, stackC));
    float *stack[UGSM_MAX_BATCH];
    const FoveaCall call = FoveaCall::pairs(n, off_x, off_y, stack);
    if (n == 1 || fovea_batch_runs_pair_by_pair(ctx)) {
        for (int b = 0; b < n; b++)
            UCHK(match_foveated_host(ctx, slot, rgbL[b], rgbR[b], W, H, stride, call.off_x[b], call.off_y[b], stackH[b], stackV[b], stackC[b], nullptr,
                                     nullptr, false));
        return UGSM_OK;
    }
    FoveaRoom room;
    UCHK(fovea_room(ctx, W, H, call.kind, n, room));
    const uint8_t *dL[UGSM_MAX_BATCH], *dR[UGSM_MAX_BATCH];
    UCHK(stage_in_batch(ctx, *s, n, rgbL, rgbR, W, H, stride, dL, dR));
    size_t at[UGSM_MAX_BATCH];  // (behind the states: the n stacks)
    for (int b = 0; b < n; b++) at[b] = room.part(room.stack);
    UCHK(fovea_grow(ctx, *s, W, H, call, room));
    for (int b = 0; b < n; b++) stack[b] = s->hout + at[b];
    UCHK(enqueue_foveated(ctx, *s, slot, dL, dR, W, H, stride, call));
    for (int b = 0; b < n; b++) UCHK(download_stack(ctx, *s, stack[b], room.plane, stackH[b], stackV[b], stackC[b]));
    return mark_done(ctx, *s);
}

}  // extern "C"
