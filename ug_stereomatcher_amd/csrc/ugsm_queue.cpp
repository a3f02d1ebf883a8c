// ugsm_queue.cpp -- the queue of include/ugsm.h: ugsm_enqueue_* / ugsm_flush / ugsm_next_done.
//
// The library owns the slots: it forms calls from the backlog ("batch what has piled up", staggered first round), deals them onto the
// slots in rotation and reports completions in enqueue order.  This is the host logic that produced the throughput figures of rounds 3
// and 4 from inside bench.py (plan_calls / run / submit), moved behind the C-ABI so that the C++ node's topic path
// (/root/reference/src/gpu_matcher/UG_GPU_matcher.cpp:126-185,414-494 -- one blocking match() per callback of a single-threaded
// ros::spin, :749-752) gets the same pipeline from three calls.  Written against the public slot-level entry points only -- and, for the
// pairs that carry a cloud (ugsm_enqueue_*_cloud*) or are checked (ugsm_enqueue_full_checked*), function pointers of CtxHooks that the
// runtime sets in ugsm_create: no symbol of the runtime's cloud work or of its checked call is named here, so the file still links against a
// runtime that has none (tests/fake_runtime.cpp).
#include "ugsm_internal.hpp"

#include <time.h>  // (no HIP header: the queue makes no HIP call -- tests/test_queue_host.py builds this file with g++ against a fake runtime)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

using namespace ugsm;

namespace {

enum Mode { M_FULL = 0, M_FOVEA = 1 };
enum Mem { MEM_DEVICE = 0, MEM_PINNED = 1, MEM_MANAGED = 2 };

struct Pinned {  // page-locked memory the queue owns (pinned_room)
    void *p = nullptr;
    size_t bytes = 0;
};
// page-locked staging of one managed pair: both images in, the result planes out, the cloud out (ugsm_enqueue_*_cloud_managed: grown to
// the largest cloud a pair in this buffer has stored, when the pair's count is known -- never to the dense size up front)
struct Managed {
    Pinned in, out, cloud;
    bool busy = false;
};

// One pair, as its entry point states it -- the leading members, in the order an entry point lists them -- and as the queue keeps it.
struct Item {
    int mode, mem;
    const uint8_t *L, *R;  // (a managed pair: the caller's images until the pair is accepted, its staging from then on: stage_managed)
    int W, H, stride, off_x, off_y;
    float *out[5];  // device: out[0] = d_out / d_stack, out[3], out[4] = d_pyrL / d_pyrR; host: H, V, C planes (+ pyramid stacks)
    uint64_t tag;
    bool want_pyr = false;  // a managed foveated pair asks for its pyramid stacks
    // the cloud job of a pair enqueued with ugsm_enqueue_*_cloud*: the device kind's cloud buffers, and the spec as it was at enqueue
    bool has_cloud = false;
    void *points = nullptr;
    long long cap = 0;
    long long *count = nullptr, *level_counts = nullptr;
    ugsm_queue_cloud spec{};
    int fmt = 0;  // the input format the pair was enqueued in (ugsm_set_input_format at the time of its ugsm_enqueue_*)
    unsigned long long seq = 0;
    int managed = -1;  // index into Queue::pool, or -1
    // a checked pair (ugsm_enqueue_full_checked*): its own threshold, and the right camera's checked field where the pair takes it -- the
    // device kind: back[0] = d_back; managed with want_back: the three planes, carved from the staging like out[0 .. 2]
    bool checked = false, want_back = false;
    float tau = 0.0f;
    float *back[3] = {nullptr, nullptr, nullptr};
    bool pyr() const { return out[3] != nullptr || out[4] != nullptr; }
    // pairs of one call: one mode, one kind of memory, one geometry, one input format; host calls with pyramid stacks go out alone (the
    // batched host entry point has none); all with a cloud, of one byte-equal spec, or all without; all checked, with one bit-equal tau, or
    // none (whether a checked pair takes its back field is the pair's own: the call has an entry per pair for it)
    bool same_kind(const Item &o) const
    {
        return mode == o.mode && mem == o.mem && W == o.W && H == o.H && stride == o.stride && fmt == o.fmt &&
               !(mem != MEM_DEVICE && (pyr() || o.pyr())) && has_cloud == o.has_cloud && (!has_cloud || memcmp(&spec, &o.spec, sizeof spec) == 0) &&
               checked == o.checked && (!checked || memcmp(&tau, &o.tau, sizeof tau) == 0);
    }
};

struct Call {
    int slot = 0, status = UGSM_OK;
    long long index = 0;
    std::vector<Item> items;
    size_t reported = 0;  // pairs already moved to the done list (retire_front can be resumed after an allocation failure)
    // A managed cloud call completes in two steps (the size of a compact cloud is only known on the device).  phase 0: the match, the clouds
    // and the download of their counts are on the slot's stream; when the slot is seen idle the finish hook reads the counts and enqueues
    // the clouds' device-to-host copies there -- phase 1, the slot busy again; the call is retired when that has drained.  (A call whose
    // submit failed, or whose slot reported an error, has no second step.)  Every other call is in phase 1 from the start.
    int phase = 1;
    std::vector<ugsm_cloud_result> clouds;  // managed cloud calls: what ugsm_done_cloud reports for each pair
    std::vector<ugsm_checked_result> checked;  // checked calls: what ugsm_done_checked reports for each pair (the counts: read_marks) ...
    bool marks_read = false;                   // ... once, when the call is retired
};

struct Done {
    ugsm_completion c;
    int managed;  // the managed buffer the completion lends, or -1
    bool has_cloud;  // a managed cloud pair of a call that succeeded: ...
    ugsm_cloud_result cloud;  // ... what ugsm_done_cloud reports after this completion
    bool checked;  // a checked pair of a call that succeeded: ...
    ugsm_checked_result chk;  // ... what ugsm_done_checked reports after this completion
};

struct Queue {
    std::deque<Item> waiting;
    std::deque<Call> flight;             // in dispatch order; retired from the front
    std::deque<Done> done;               // retired, not yet fetched
    std::vector<Managed> pool;
    std::vector<int> lent;               // managed buffers the last ugsm_next_done lent to the host
    bool last_has_cloud = false;         // the pair the last ugsm_next_done reported carried a managed cloud: ...
    ugsm_cloud_result last_cloud{};      // ... this one (ugsm_done_cloud)
    bool last_checked = false;           // ... was a checked pair of a call that succeeded: ...
    ugsm_checked_result last_chk{};      // ... this is what ugsm_done_checked answers
    unsigned long long seq = 0, flush_upto = 0;
    bool round_restarts = false;  // a flush has closed the burst: the next pair enqueued opens a new staggered round
    long long calls = 0, calls_since_idle = 0;
    int next_slot = 0;
    std::vector<char> slot_busy;
    int outstanding() const
    {
        size_t n = waiting.size() + done.size();
        for (const Call &c : flight) n += c.items.size() - c.reported;
        return (int)n;
    }
};

long long now_ns()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (long long)ts.tv_sec * 1000000000LL + ts.tv_nsec;
}

int batch_of(const ugsm_config &cfg) { return std::min(std::max(cfg.batch, 1), UGSM_MAX_BATCH); }

void queue_free(ugsm_ctx *ctx, void *p)
{
    Queue *q = static_cast<Queue *>(p);
    for (Managed &m : q->pool)
        for (Pinned *b : {&m.in, &m.out, &m.cloud})
            if (b->p) (void)ugsm_host_free(ctx, b->p);
    delete q;
}

// at least `bytes` of page-locked memory in b; the old contents are not kept.  false: out of memory -- b is empty and ugsm_host_alloc has
// set the message
bool pinned_room(ugsm_ctx *ctx, Pinned &b, size_t bytes)
{
    if (b.bytes >= bytes) return true;
    if (b.p) (void)ugsm_host_free(ctx, b.p);
    b = Pinned{};
    void *p = nullptr;
    if (ugsm_host_alloc(ctx, &p, (long long)bytes) != UGSM_OK) return false;
    b = Pinned{p, bytes};
    return true;
}

Queue *queue_of(ugsm_ctx *ctx)
{
    CtxHooks &h = ctx_hooks(ctx);
    if (!h.queue) {
        // (nothing is thrown from here: ugsm_enqueue_* and ugsm_queue_depth ask outside a no_throw body, and the members' own
        // constructors allocate)
        Queue *q = nullptr;
        try {
            q = new Queue();
            q->slot_busy.assign((size_t)ctx_config(ctx).slots, 0);
        } catch (...) {
            delete q;
            return nullptr;
        }
        h.queue = q;
        h.queue_free = queue_free;
    }
    return static_cast<Queue *>(h.queue);
}

void update_busy(ugsm_ctx *ctx, Queue *q) { ctx_hooks(ctx).queue_busy = !(q->waiting.empty() && q->flight.empty() && q->done.empty()); }

// A checked call has drained: what its check marked, per pair and direction, from the runtime (the slot still holds the call's counts: it is
// not used again before the call is retired).  A call that failed has none.
void read_marks(ugsm_ctx *ctx, Call &c)
{
    if (c.marks_read || c.checked.empty()) return;
    c.marks_read = true;
    if (c.status != UGSM_OK) return;
    CtxHooks &h = ctx_hooks(ctx);
    long long fwd[UGSM_MAX_BATCH] = {0}, back[UGSM_MAX_BATCH] = {0};
    const int st = h.checked_marked ? h.checked_marked(ctx, c.slot, (int)c.items.size(), fwd, back) : UGSM_ERR_STATE;
    if (st != UGSM_OK) {
        c.status = st;
        return;
    }
    for (size_t b = 0; b < c.checked.size(); b++) {
        const Item &it = c.items[b];
        ugsm_checked_result &r = c.checked[b];
        for (int k = 0; k < 3; k++) r.back[k] = it.mem == MEM_MANAGED && it.want_back ? it.back[k] : nullptr;
        r.marked_fwd = fwd[b];
        r.marked_back = back[b];
    }
}

// the oldest call in flight is complete: its pairs move to the done list
void retire_front(ugsm_ctx *ctx, Queue *q)
{
    Call &c = q->flight.front();
    const long long t = now_ns();
    read_marks(ctx, c);
    for (; c.reported < c.items.size(); c.reported++) {  // (push_back may throw: what has been reported is not reported again)
        const Item &it = c.items[c.reported];
        ugsm_completion d{};
        d.tag = it.tag;
        d.status = c.status;
        d.slot = c.slot;
        d.call_pairs = (int)c.items.size();
        d.call_index = c.index;
        d.done_ns = t;
        if (it.mem == MEM_MANAGED)
            for (int k = 0; k < 5; k++) d.result[k] = it.out[k];
        const bool cloud = it.has_cloud && it.mem == MEM_MANAGED && c.status == UGSM_OK && c.reported < c.clouds.size();
        const bool chk = it.checked && c.status == UGSM_OK && c.reported < c.checked.size();
        q->done.push_back(Done{d, it.managed, cloud, cloud ? c.clouds[c.reported] : ugsm_cloud_result{}, chk, chk ? c.checked[c.reported] : ugsm_checked_result{}});
    }
    q->slot_busy[(size_t)c.slot] = 0;
    q->flight.pop_front();
}

// page-locked room for the cloud of pair `pair` of the call being finished (CtxHooks::cloud_finish asks once the pair's count is known)
struct StagingFor {
    ugsm_ctx *ctx;
    Queue *q;
    Call *c;
};
void *cloud_staging(void *user, int pair, long long bytes)
{
    StagingFor *u = static_cast<StagingFor *>(user);
    if (pair < 0 || (size_t)pair >= u->c->items.size() || bytes < 0) return nullptr;
    const int idx = u->c->items[(size_t)pair].managed;
    if (idx < 0) return nullptr;
    Pinned &cloud = u->q->pool[(size_t)idx].cloud;
    return pinned_room(u->ctx, cloud, (size_t)bytes) ? cloud.p : nullptr;
}

// The slot of a managed cloud call in phase 0 has drained (st: what ugsm_poll / ugsm_wait answered): the finish hook -- once per call -- puts
// the clouds' copies on the slot's stream.  A call that failed has nothing to fetch; whatever the hook did enqueue before it failed is
// drained like any other work before the pairs are reported.
void cloud_second_step(ugsm_ctx *ctx, Queue *q, Call &c, int st)
{
    c.phase = 1;
    if (st != UGSM_OK && c.status == UGSM_OK) c.status = st;
    if (c.status != UGSM_OK) return;
    CtxHooks &h = ctx_hooks(ctx);
    StagingFor user{ctx, q, &c};
    h.queue_calling = true;
    h.queue_more = true;  // (copies only: the slot does not become a call that has the chip to itself)
    const int fst = h.cloud_finish ? h.cloud_finish(ctx, c.slot, (int)c.items.size(), c.clouds.data(), cloud_staging, &user) : UGSM_ERR_STATE;
    h.queue_calling = false;
    h.queue_more = false;
    if (fst != UGSM_OK) c.status = fst;
}

// Retires every call at the front of the flight list that has finished (never blocks).  A call whose submit FAILED is drained like any
// other before its pairs are reported: a submit can fail after work has gone onto the slot's stream (out of memory for the staging of a
// later phase, a launch error mid-call), and a completion tells the host that its input and result buffers -- or the managed staging
// buffer the library lends next -- are free.  The submit's status is the one reported.
void reap(ugsm_ctx *ctx, Queue *q)
{
    // managed cloud calls whose first step has drained start their second, wherever they are in the flight list: a later call's clouds
    // come down while the calls before it are still matching
    for (Call &c : q->flight) {
        if (c.phase != 0) continue;
        const int st = ugsm_poll(ctx, c.slot);
        if (st != UGSM_PENDING) cloud_second_step(ctx, q, c, st);
    }
    while (!q->flight.empty()) {
        Call &c = q->flight.front();
        if (c.phase == 0) break;
        const int st = ugsm_poll(ctx, c.slot);
        if (st == UGSM_PENDING) break;
        if (st != UGSM_OK && c.status == UGSM_OK) c.status = st;
        retire_front(ctx, q);
    }
}

// blocks until the oldest call in flight has finished (or, its submit having failed, until what it did enqueue has drained), and retires it
void wait_front(ugsm_ctx *ctx, Queue *q)
{
    Call &c = q->flight.front();
    if (c.phase == 0) cloud_second_step(ctx, q, c, ugsm_wait(ctx, c.slot));
    const int st = ugsm_wait(ctx, c.slot);
    if (st != UGSM_OK && c.status == UGSM_OK) c.status = st;
    retire_front(ctx, q);
}

// A slot without a call in flight, in rotation order from next_slot; -1 if every slot is busy.  A slot whose call has finished but is
// not at the front of the flight list (calls may finish out of order) stays busy until the calls before it have been retired: results
// are reported in enqueue order, and the slot's buffers belong to its call until then.
int free_slot(const Queue *q)
{
    const int n = (int)q->slot_busy.size();
    for (int k = 0; k < n; k++) {
        const int s = (q->next_slot + k) % n;
        if (!q->slot_busy[(size_t)s]) return s;
    }
    return -1;
}

// the pairs of a call, as columns: what the ugsm_submit_*_batch entry points take
struct Columns {
    const uint8_t *L[UGSM_MAX_BATCH], *R[UGSM_MAX_BATCH];
    int off_x[UGSM_MAX_BATCH], off_y[UGSM_MAX_BATCH];
    float *out[5][UGSM_MAX_BATCH];  // (Item::out, transposed)
    bool any_pyr = false;
};

// a pair's part of the call the cloud hook takes: a managed pair has its planes where a device pair has its d_out / d_stack
CloudJob cloud_job(const Item &it)
{
    float *const none = nullptr;
    if (it.mem == MEM_MANAGED) return CloudJob{it.L, it.R, it.off_x, it.off_y, none, {it.out[0], it.out[1], it.out[2]}, it.points, it.cap, it.count, it.level_counts};
    return CloudJob{it.L, it.R, it.off_x, it.off_y, it.out[0], {none, none, none}, it.points, it.cap, it.count, it.level_counts};
}

// a pair's part of the call the checked hook takes
CheckedJob checked_job(const Item &it)
{
    float *const none = nullptr;
    if (it.mem == MEM_MANAGED)
        return CheckedJob{it.L, it.R, none, none, {it.out[0], it.out[1], it.out[2]}, {it.back[0], it.back[1], it.back[2]}, nullptr, 0, nullptr};
    return CheckedJob{it.L, it.R, it.out[0], it.back[0], {none, none, none}, {none, none, none}, it.points, it.cap, it.count};
}

// One library call for the first n waiting pairs on `slot`.  more: other calls follow this one closely -- pairs wait behind it, or it filled
// up without a flush (a host that submits faster than the chip matches): the runtime then takes the call to share the chip whatever the
// other slots are doing at this instant (call_alone, ugsm_policy.cpp).
void dispatch(ugsm_ctx *ctx, Queue *q, int n, int slot, bool more)
{
    // the call's place in the flight list first: everything that can run out of host memory happens before anything reaches the GPU,
    // and a call that has reached the GPU is always on the list
    q->flight.emplace_back();
    Call &c = q->flight.back();
    try {
        c.items.assign(q->waiting.begin(), q->waiting.begin() + n);
        if (c.items[0].has_cloud && c.items[0].mem == MEM_MANAGED) c.clouds.resize((size_t)n);
        if (c.items[0].checked) c.checked.resize((size_t)n);
    } catch (...) {
        q->flight.pop_back();
        throw;  // (to the entry point's no_throw; the pairs still wait)
    }
    c.slot = slot;
    c.index = q->calls++;
    q->waiting.erase(q->waiting.begin(), q->waiting.begin() + n);
    const Item &f = c.items[0];
    const bool fovea = f.mode == M_FOVEA, host = f.mem != MEM_DEVICE;
    Columns p;
    CloudCall cc{fovea, f.mem == MEM_MANAGED, n, f.W, f.H, f.stride, &f.spec, {}};  // (sent only if the pairs carry a cloud)
    for (int b = 0; b < n; b++) {
        const Item &it = c.items[(size_t)b];
        p.L[b] = it.L;
        p.R[b] = it.R;
        p.off_x[b] = it.off_x;
        p.off_y[b] = it.off_y;
        for (int k = 0; k < 5; k++) p.out[k][b] = it.out[k];
        p.any_pyr = p.any_pyr || it.pyr();
        if (f.has_cloud) cc.job[b] = cloud_job(it);
    }
    float *const *o0 = p.out[0], *const *o1 = p.out[1], *const *o2 = p.out[2], *const *pl = p.out[3], *const *pr = p.out[4];
    CtxHooks &h = ctx_hooks(ctx);
    h.queue_calling = true;
    h.queue_more = more;
    // the call reads its images in the format its pairs were enqueued in, whatever the host has set since
    const int host_fmt = h.input_format;
    h.input_format = f.fmt;
    int st;
    if (f.checked) {  // both directions of the call's pairs in lockstep, checked with the pairs' tau, and their clouds if they carry one: the runtime's hook
        CheckedCall kc{f.mem == MEM_MANAGED, n, f.W, f.H, f.stride, f.tau, f.has_cloud ? &f.spec : nullptr, {}};
        for (int b = 0; b < n; b++) kc.job[b] = checked_job(c.items[(size_t)b]);
        st = h.checked_submit ? h.checked_submit(ctx, slot, &kc) : UGSM_ERR_STATE;
        if (f.has_cloud && kc.managed) c.phase = 0;  // (the managed clouds' second step: as below)
    } else if (f.has_cloud) {  // the match and the clouds of the call's pairs: the runtime's hook
        st = h.cloud_submit ? h.cloud_submit(ctx, slot, &cc) : UGSM_ERR_STATE;
        if (cc.managed) c.phase = 0;  // (a failed submit too: cloud_second_step sees the status once the slot has drained)
    } else if (!fovea && !host) {
        st = n == 1 ? ugsm_submit_full(ctx, slot, p.L[0], p.R[0], f.W, f.H, f.stride, o0[0]) : ugsm_submit_full_batch(ctx, slot, n, p.L, p.R, f.W, f.H, f.stride, o0);
    } else if (fovea && !host) {
        st = n == 1 ? ugsm_submit_foveated(ctx, slot, p.L[0], p.R[0], f.W, f.H, f.stride, p.off_x[0], p.off_y[0], o0[0], pl[0], pr[0])
                    : ugsm_submit_foveated_batch(ctx, slot, n, p.L, p.R, f.W, f.H, f.stride, p.off_x, p.off_y, o0, p.any_pyr ? pl : nullptr,
                                                 p.any_pyr ? pr : nullptr);
    } else if (!fovea) {
        st = n == 1 ? ugsm_submit_full_host(ctx, slot, p.L[0], p.R[0], f.W, f.H, f.stride, o0[0], o1[0], o2[0])
                    : ugsm_submit_full_batch_host(ctx, slot, n, p.L, p.R, f.W, f.H, f.stride, o0, o1, o2);
    } else {
        st = n == 1 ? ugsm_submit_foveated_host(ctx, slot, p.L[0], p.R[0], f.W, f.H, f.stride, p.off_x[0], p.off_y[0], o0[0], o1[0], o2[0], pl[0], pr[0])
                    : ugsm_submit_foveated_batch_host(ctx, slot, n, p.L, p.R, f.W, f.H, f.stride, p.off_x, p.off_y, o0, o1, o2);
    }
    h.input_format = host_fmt;
    h.queue_calling = false;
    h.queue_more = false;
    c.status = st;  // (a call that failed to enqueue: its pairs are reported with this status once the slot has drained, reap / wait_front)
    q->slot_busy[(size_t)slot] = 1;
    q->next_slot = (slot + 1) % (int)q->slot_busy.size();
    q->calls_since_idle++;
}

// Forms and sends calls from the backlog.  may_block: a call that is full may wait for the slot of the oldest call in flight
// (ugsm_enqueue_*: back-pressure); otherwise only free slots are used.  How a call went is reported with its pairs (ugsm_completion.status),
// never through the entry point that happened to send it: that call may hold other pairs than the one just enqueued.
void pump(ugsm_ctx *ctx, Queue *q, bool may_block)
{
    const ugsm_config &cfg = ctx_config(ctx);
    while (!q->waiting.empty()) {
        reap(ctx, q);
        if (q->round_restarts && q->waiting.front().seq > q->flush_upto) {
            // the pairs before the last flush have all gone out: what arrived after it is a new burst, staggered again (a host's flush is
            // the one event that says "the pipe is about to drain" without depending on how fast the GPU happens to be)
            q->round_restarts = false;
            q->calls_since_idle = 0;
        }
        const int target = queue_target(batch_of(cfg), cfg.slots, q->calls_since_idle);
        const Item &f = q->waiting.front();
        const int cap = (f.mem != MEM_DEVICE && f.pyr()) ? 1 : target;
        int n = 0;
        bool kind_ends = false;  // a pair of another kind waits behind the group: the group goes out as it is
        for (const Item &it : q->waiting) {
            if (n >= cap) break;
            if (!it.same_kind(f)) {
                kind_ends = true;
                break;
            }
            n++;
        }
        if (n < 1) n = 1;  // (a host pair with pyramid stacks is not the same kind as itself: alone)
        const bool full = n >= cap || kind_ends;
        if (!full) {
            // only the pairs a flush has covered go out in a call that is not full
            int m = 0;
            while (m < n && q->waiting[(size_t)m].seq <= q->flush_upto) m++;
            if (m == 0) break;
            n = m;
        }
        int slot = free_slot(q);
        if (slot < 0) {
            if (!(full && may_block) || q->flight.empty()) break;
            wait_front(ctx, q);
            reap(ctx, q);
            slot = free_slot(q);
            if (slot < 0) break;
        }
        const bool by_itself = full && !kind_ends && cap > 1 && q->waiting[(size_t)n - 1].seq > q->flush_upto;
        dispatch(ctx, q, n, slot, (int)q->waiting.size() > n || by_itself);
    }
    update_busy(ctx, q);
}

int check_geometry(ugsm_ctx *ctx, int W, int H, int stride, bool fovea, const void *L, const void *R)
{
    const ugsm_config &cfg = ctx_config(ctx);
    int w[UGSM_MAX_LEVELS], h[UGSM_MAX_LEVELS];
    const int st = ugsm_level_dims(W, H, cfg.levels, w, h);
    if (st != UGSM_OK) return ctx_fail(ctx, st, "ugsm_enqueue_*: bad image size for the context's pyramid");
    const int is = input_image_status(ctx_hooks(ctx).input_format, W, stride, L, R);
    if (is == UGSM_ERR_SIZE_MISMATCH) return ctx_fail(ctx, is, "ugsm_enqueue_*: stride < bytes per pixel of the input format * W");
    if (is != UGSM_OK) return ctx_fail(ctx, is, "ugsm_enqueue_*: a float image's pointers and stride must be 4-byte aligned");
    if (fovea && cfg.fovea_levels < 2) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_foveated*: the context has no fovea levels");
    return UGSM_OK;
}

// (slots + 1) x batch pairs may be outstanding -- waiting, in flight or finished and not yet fetched.  In-flight and waiting pairs alone
// never reach that number (a full call goes out, or waits for its slot, inside the enqueue that completes it), so a full queue means
// completions the host has not fetched: refuse instead of letting it recycle a result buffer it has not read.
int room(ugsm_ctx *ctx, const Queue *q)
{
    const ugsm_config &cfg = ctx_config(ctx);
    if (q->outstanding() < (cfg.slots + 1) * batch_of(cfg)) return UGSM_OK;
    return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_enqueue_*: (slots + 1) x batch pairs are outstanding and completions wait to be fetched: call ugsm_next_done first");
}

// a managed buffer with room for `in_bytes` of images and `out_floats` of results; -1: out of memory (ugsm_host_alloc has set the message)
int managed_get(ugsm_ctx *ctx, Queue *q, size_t in_bytes, size_t out_floats)
{
    const size_t out_bytes = out_floats * sizeof(float);
    int idx = -1;
    for (size_t k = 0; k < q->pool.size(); k++)
        if (!q->pool[k].busy && (idx < 0 || (q->pool[k].in.bytes >= in_bytes && q->pool[k].out.bytes >= out_bytes))) idx = (int)k;
    if (idx < 0) {
        q->pool.emplace_back();
        idx = (int)q->pool.size() - 1;
    }
    Managed &m = q->pool[(size_t)idx];
    if (!pinned_room(ctx, m.in, in_bytes) || !pinned_room(ctx, m.out, out_bytes)) return -1;
    m.busy = true;
    return idx;
}

// What is a managed pair's own, once the queue has room for it: a staging buffer, the images into it -- compacted to rows of bytes-per-pixel
// x W bytes; after this the caller's memory is not touched again -- and the pair's images and results carved from it.
int stage_managed(ugsm_ctx *ctx, Queue *q, Item &it)
{
    const ugsm_config &cfg = ctx_config(ctx);
    const bool planes = !it.has_cloud || it.spec.want_planes != 0;  // (a cloud pair that does not want its planes has no room for them)
    const bool pyr = it.mode == M_FOVEA && it.want_pyr;
    const size_t row = (size_t)input_bpp(ctx_hooks(ctx).input_format) * it.W, img = (row * (size_t)it.H + 255) & ~(size_t)255;
    size_t plane = (size_t)it.W * it.H;
    if (it.mode == M_FOVEA) {
        int fw = 0, fh = 0;
        (void)ugsm_fovea_dims(it.W, it.H, cfg.levels, cfg.fovea_levels, &fw, &fh);
        plane = (size_t)cfg.fovea_levels * fw * fh;
    }
    int idx = -1;
    const int grown = no_throw(ctx, "ugsm_enqueue_*_managed: out of host memory", [&]() -> int {
        idx = managed_get(ctx, q, 2 * img, (planes ? 3 * plane : 0) + (pyr ? 6 * plane : 0) + (it.want_back ? 3 * plane : 0));
        return UGSM_OK;
    });
    if (grown != UGSM_OK || idx < 0) return UGSM_ERR_NOMEM;  // (ugsm_host_alloc has set the message)
    uint8_t *in = static_cast<uint8_t *>(q->pool[(size_t)idx].in.p);
    float *out = static_cast<float *>(q->pool[(size_t)idx].out.p);
    for (int side = 0; side < 2; side++) {
        const uint8_t *src = side == 0 ? it.L : it.R;
        uint8_t *dst = in + side * img;
        if ((size_t)it.stride == row) {
            ctx_host_copy(ctx, dst, src, row * (size_t)it.H);
        } else {
            for (int y = 0; y < it.H; y++) memcpy(dst + (size_t)y * row, src + (size_t)y * it.stride, row);
        }
    }
    it.L = in;
    it.R = in + img;
    it.stride = (int)row;
    for (int k = 0; k < 3; k++) it.out[k] = planes ? out + k * plane : nullptr;
    it.out[3] = pyr ? out + 3 * plane : nullptr;
    it.out[4] = pyr ? out + 6 * plane : nullptr;
    for (int k = 0; k < 3; k++) it.back[k] = it.want_back ? out + ((planes ? 3 : 0) + k) * plane : nullptr;  // (a checked pair is full-mode: no stacks)
    it.managed = idx;
    return UGSM_OK;
}

// What every ugsm_enqueue_*_cloud* checks of its spec and, the device kind, of its cloud buffers: the slot-level cloud calls' own rules
// (ugsm_internal.hpp), made when the pair is enqueued so that a bad pair is rejected and never reported
int check_cloud(ugsm_ctx *ctx, const ugsm_queue_cloud *spec, const Item &it)
{
    const int W = it.W, H = it.H;
    if (!spec) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_*_cloud*: null spec");
    const ugsm_cloud_params &p = spec->params;
    if (W < 1 || H < 1 || (long long)W * H > kMaxPixels) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_*_cloud*: bad image size");
    if (!cloud_records_ok(p)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_*_cloud*: sampling < 1 or an unknown record format");
    if (!keep_window_ok(p.min_conf, p.z_min, p.z_max, true))
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_*_cloud*: a NaN min_conf / z_min / z_max, or z_min > z_max");
    if (spec->max_points < 0) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_*_cloud*: max_points < 0");
    if (it.mem == MEM_DEVICE && (!it.points || !it.count || it.cap < 0 || ((uintptr_t)it.points & 15) || ((uintptr_t)it.count & 7) || ((uintptr_t)it.level_counts & 7)))
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_*_cloud: a null or misaligned cloud buffer, or cap_points < 0");
    if (!ctx_hooks(ctx).cloud_submit || !ctx_hooks(ctx).cloud_finish) return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_enqueue_*_cloud*: this runtime makes no clouds");
    return UGSM_OK;
}
// What every ugsm_enqueue_full_checked* checks of its threshold and of the context: what ugsm_submit_full_checked would refuse when the pair's
// call goes out (full_checked_check, ugsm_full.cpp), made when the pair is enqueued so that a bad pair is rejected and never reported
int check_checked(ugsm_ctx *ctx, const Item &it)
{
    const ugsm_config &cfg = ctx_config(ctx);
    if (!(it.tau > 0.0f)) return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_full_checked*: tau must be > 0");
    if (cfg.early_exit_threshold > 0.0f || cfg.kernel_path == 1)
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, "ugsm_enqueue_full_checked*: not with early_exit_threshold > 0 or kernel_path 1");
    if (!ctx_hooks(ctx).checked_submit || !ctx_hooks(ctx).checked_marked)
        return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_enqueue_full_checked*: this runtime has no checked full-mode call");
    return UGSM_OK;
}
Item as_checked(Item it, float tau, float *d_back, bool want_back = false)
{
    it.checked = true;
    it.tau = tau;
    it.back[0] = d_back;
    it.want_back = want_back;
    return it;
}
Item with_cloud(Item it, void *points = nullptr, long long cap = 0, long long *count = nullptr, long long *level_counts = nullptr)
{
    it.has_cloud = true;
    it.points = points;
    it.cap = cap;
    it.count = count;
    it.level_counts = level_counts;
    return it;
}

const char kNoMem[] = "ugsm_enqueue_*: out of host memory";

// The one way in.  `it`: the pair as its entry point `name` states it; required: how many of its leading result pointers must be set; spec:
// the cloud spec of a pair made with_cloud.  The refusals in the order every entry point has had them -- a refused pair is never reported --,
// then the pair is accepted: whatever happens to its call comes out of ugsm_next_done.
int enqueue_pair(ugsm_ctx *ctx, const char *name, Item it, int required, const ugsm_queue_cloud *spec = nullptr)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    char msg[256];
    bool null = !it.L || !it.R;
    for (int k = 0; k < required; k++) null = null || !it.out[k];
    if (null) {
        snprintf(msg, sizeof msg, "%s: null buffer", name);
        return ctx_fail(ctx, UGSM_ERR_BAD_ARG, it.mem == MEM_MANAGED ? "ugsm_enqueue_*_managed: null image" : msg);
    }
    const int g = check_geometry(ctx, it.W, it.H, it.stride, it.mode == M_FOVEA, it.L, it.R);
    if (g != UGSM_OK) return g;
    if (it.mem == MEM_PINNED) {
        bool pinned = host_pinned(it.L) && host_pinned(it.R);
        for (float *o : it.out) pinned = pinned && (!o || host_pinned(o));
        if (!pinned) {
            snprintf(msg, sizeof msg, "%s: every host buffer must be page-locked (ugsm_host_alloc, hipHostMalloc or hipHostRegister); ugsm_enqueue_%s_managed takes any memory",
                     name, it.mode == M_FULL ? "full" : "foveated");
            return ctx_fail(ctx, UGSM_ERR_BAD_ARG, msg);
        }
    }
    if (it.checked) {
        const int ks = check_checked(ctx, it);
        if (ks != UGSM_OK) return ks;
    }
    if (it.has_cloud) {
        if (ctx_hooks(ctx).lens_set) {  // (the queue's pair records do not capture the lens: include/ugsm.h, "lens distortion")
            snprintf(msg, sizeof msg, "%s: a lens is set (ugsm_set_lens) and the queue's clouds do not honour it; switch it off or take the cloud with ugsm_point_cloud*", name);
            return ctx_fail(ctx, UGSM_ERR_STATE, msg);
        }
        const int cs = check_cloud(ctx, spec, it);
        if (cs != UGSM_OK) return cs;
        it.spec = *spec;  // (copied now: the call is formed later)
        it.spec.reserved = 0;
    }
    Queue *q = queue_of(ctx);
    if (!q) return ctx_fail(ctx, UGSM_ERR_NOMEM, kNoMem);
    const int r = room(ctx, q);
    if (r != UGSM_OK) return r;
    if (it.mem == MEM_MANAGED) {  // (only now: a pair the queue refuses is not copied)
        const int ms = stage_managed(ctx, q, it);
        if (ms != UGSM_OK) return ms;
    }
    const int st = no_throw(ctx, kNoMem, [&]() -> int {
        it.seq = q->seq + 1;
        it.fmt = ctx_hooks(ctx).input_format;  // (captured now: the call is formed later)
        q->waiting.push_back(it);
        q->seq = it.seq;
        ctx_hooks(ctx).queue_busy = true;
        // a pump that ran out of host memory leaves the pairs waiting for the next entry point's pump: that is not a rejection
        (void)no_throw(ctx, kNoMem, [&]() -> int {
            pump(ctx, q, true);
            return UGSM_OK;
        });
        update_busy(ctx, q);
        return UGSM_OK;
    });
    if (st != UGSM_OK && it.managed >= 0) q->pool[(size_t)it.managed].busy = false;  // (rejected: the staging buffer is free again)
    return st;
}

int next_done(ugsm_ctx *ctx, ugsm_completion *out, int block)
{
    Queue *q = queue_of(ctx);
    if (!q) return ctx_fail(ctx, UGSM_ERR_NOMEM, "ugsm_next_done: out of host memory");
    for (int idx : q->lent) q->pool[(size_t)idx].busy = false;  // what the previous call lent comes back
    q->lent.clear();
    if (block && q->flush_upto != q->seq) {
        q->flush_upto = q->seq;
        q->round_restarts = true;
    }
    for (;;) {
        reap(ctx, q);
        pump(ctx, q, false);  // (a slot may just have come free for pairs that wait)
        if (!q->done.empty()) break;
        if (q->flight.empty() && q->waiting.empty()) {
            update_busy(ctx, q);
            return UGSM_EMPTY;
        }
        if (!block) {
            update_busy(ctx, q);
            return UGSM_PENDING;
        }
        if (q->flight.empty()) {
            // pairs wait and no call is in flight, yet pump sent nothing: cannot happen (every slot is free); do not spin
            update_busy(ctx, q);
            return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_next_done: the queue cannot make progress");
        }
        wait_front(ctx, q);
    }
    const int m = q->done.front().managed;
    if (m >= 0) q->lent.push_back(m);  // (before the completion leaves the list: a push_back that throws loses nothing)
    *out = q->done.front().c;
    q->last_has_cloud = q->done.front().has_cloud;
    q->last_cloud = q->done.front().cloud;
    q->last_checked = q->done.front().checked;
    q->last_chk = q->done.front().chk;
    q->done.pop_front();
    // (pairs that waited for room may go out now; the slot-level entry points open up again once nothing is outstanding)
    pump(ctx, q, false);
    return UGSM_OK;
}

}  // namespace

namespace ugsm {
// call c (0-based) since the queue was idle: the first `slots` calls are staggered in size, ceil(batch (c + 2) / (slots + 1)) -- 4, 5, 7,
// 8 for batch 8 on four slots -- so that the slots do not march through the levels in phase from a drained pipe (same box, 20 pairs of
// 16 MP, batch 4: 172 against 169 pairs/s for equal calls, 162 for a descending start; profiles/r04_ab_plan.txt); every later call: batch
int queue_target(int batch, int slots, long long c)
{
    if (c >= slots) return batch;
    const long long t = ((long long)batch * (c + 2) + slots) / (slots + 1);
    return (int)std::max(1LL, std::min((long long)batch, t));
}
}  // namespace ugsm

extern "C" {

int ugsm_queue_plan(const ugsm_config *cfg_in, int n_pairs, int *sizes, int cap)
{
    ugsm_config cfg;
    if (cfg_in) cfg = *cfg_in;
    else ugsm_default_config(&cfg);
    if (n_pairs < 0 || cap < 0 || (cap > 0 && !sizes) || cfg.slots < 1) return -1;
    const int B = batch_of(cfg);
    int calls = 0, left = n_pairs;
    while (left > 0) {
        const int nb = std::min(left, queue_target(B, cfg.slots, calls));
        if (calls < cap) sizes[calls] = nb;
        calls++;
        left -= nb;
    }
    return calls;
}

int ugsm_enqueue_full(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out, uint64_t tag)
{
    return enqueue_pair(ctx, "ugsm_enqueue_full", Item{M_FULL, MEM_DEVICE, d_rgbL, d_rgbR, W, H, stride, 0, 0, {d_out}, tag}, 1);
}

int ugsm_enqueue_foveated(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int off_x, int off_y, float *d_stack,
                          float *d_pyrL, float *d_pyrR, uint64_t tag)
{
    const Item it{M_FOVEA, MEM_DEVICE, d_rgbL, d_rgbR, W, H, stride, off_x, off_y, {d_stack, nullptr, nullptr, d_pyrL, d_pyrR}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_foveated", it, 1);
}

int ugsm_enqueue_full_host(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float *dispH, float *dispV, float *dispC,
                           uint64_t tag)
{
    return enqueue_pair(ctx, "ugsm_enqueue_full_host", Item{M_FULL, MEM_PINNED, rgbL, rgbR, W, H, stride, 0, 0, {dispH, dispV, dispC}, tag}, 3);
}

int ugsm_enqueue_foveated_host(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y, float *stackH,
                               float *stackV, float *stackC, float *pyrL, float *pyrR, uint64_t tag)
{
    const Item it{M_FOVEA, MEM_PINNED, rgbL, rgbR, W, H, stride, off_x, off_y, {stackH, stackV, stackC, pyrL, pyrR}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_foveated_host", it, 3);
}

int ugsm_enqueue_full_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, uint64_t tag)
{
    return enqueue_pair(ctx, "ugsm_enqueue_full_managed", Item{M_FULL, MEM_MANAGED, rgbL, rgbR, W, H, stride, 0, 0, {}, tag}, 0);
}

int ugsm_enqueue_foveated_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y, int want_pyramids,
                                  uint64_t tag)
{
    const Item it{M_FOVEA, MEM_MANAGED, rgbL, rgbR, W, H, stride, off_x, off_y, {}, tag, want_pyramids != 0};
    return enqueue_pair(ctx, "ugsm_enqueue_foveated_managed", it, 0);
}

int ugsm_enqueue_full_cloud(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out,
                            const ugsm_queue_cloud *spec, void *d_points, long long cap_points, long long *d_count, uint64_t tag)
{
    const Item it{M_FULL, MEM_DEVICE, d_rgbL, d_rgbR, W, H, stride, 0, 0, {d_out}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_full_cloud", with_cloud(it, d_points, cap_points, d_count), 1, spec);
}

int ugsm_enqueue_foveated_cloud(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, int off_x, int off_y,
                                float *d_stack, const ugsm_queue_cloud *spec, void *d_points, long long cap_points, long long *d_count,
                                long long *d_level_counts, uint64_t tag)
{
    const Item it{M_FOVEA, MEM_DEVICE, d_rgbL, d_rgbR, W, H, stride, off_x, off_y, {d_stack}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_foveated_cloud", with_cloud(it, d_points, cap_points, d_count, d_level_counts), 1, spec);
}

int ugsm_enqueue_full_cloud_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, const ugsm_queue_cloud *spec,
                                    uint64_t tag)
{
    return enqueue_pair(ctx, "ugsm_enqueue_full_cloud_managed", with_cloud(Item{M_FULL, MEM_MANAGED, rgbL, rgbR, W, H, stride, 0, 0, {}, tag}), 0, spec);
}

int ugsm_enqueue_foveated_cloud_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, int off_x, int off_y,
                                        const ugsm_queue_cloud *spec, uint64_t tag)
{
    const Item it{M_FOVEA, MEM_MANAGED, rgbL, rgbR, W, H, stride, off_x, off_y, {}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_foveated_cloud_managed", with_cloud(it), 0, spec);
}

int ugsm_enqueue_full_checked(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out, float *d_back, float tau,
                              uint64_t tag)
{
    const Item it{M_FULL, MEM_DEVICE, d_rgbL, d_rgbR, W, H, stride, 0, 0, {d_out}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_full_checked", as_checked(it, tau, d_back), 1);
}

int ugsm_enqueue_full_checked_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float tau, int want_back, uint64_t tag)
{
    const Item it{M_FULL, MEM_MANAGED, rgbL, rgbR, W, H, stride, 0, 0, {}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_full_checked_managed", as_checked(it, tau, nullptr, want_back != 0), 0);
}

int ugsm_enqueue_full_checked_cloud(ugsm_ctx *ctx, const uint8_t *d_rgbL, const uint8_t *d_rgbR, int W, int H, int stride, float *d_out, float *d_back, float tau,
                                    const ugsm_queue_cloud *spec, void *d_points, long long cap_points, long long *d_count, uint64_t tag)
{
    const Item it{M_FULL, MEM_DEVICE, d_rgbL, d_rgbR, W, H, stride, 0, 0, {d_out}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_full_checked_cloud", with_cloud(as_checked(it, tau, d_back), d_points, cap_points, d_count), 1, spec);
}

int ugsm_enqueue_full_checked_cloud_managed(ugsm_ctx *ctx, const uint8_t *rgbL, const uint8_t *rgbR, int W, int H, int stride, float tau, int want_back,
                                            const ugsm_queue_cloud *spec, uint64_t tag)
{
    const Item it{M_FULL, MEM_MANAGED, rgbL, rgbR, W, H, stride, 0, 0, {}, tag};
    return enqueue_pair(ctx, "ugsm_enqueue_full_checked_cloud_managed", with_cloud(as_checked(it, tau, nullptr, want_back != 0)), 0, spec);
}

int ugsm_done_checked(ugsm_ctx *ctx, ugsm_checked_result *out)
{
    if (!ctx || !out) return UGSM_ERR_BAD_ARG;
    Queue *q = queue_of(ctx);
    if (!q) return ctx_fail(ctx, UGSM_ERR_NOMEM, "ugsm_done_checked: out of host memory");
    if (!q->last_checked) return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_done_checked: the last pair ugsm_next_done reported was no checked pair of a call that succeeded");
    *out = q->last_chk;
    return UGSM_OK;
}

int ugsm_done_cloud(ugsm_ctx *ctx, ugsm_cloud_result *out)
{
    if (!ctx || !out) return UGSM_ERR_BAD_ARG;
    Queue *q = queue_of(ctx);
    if (!q) return ctx_fail(ctx, UGSM_ERR_NOMEM, "ugsm_done_cloud: out of host memory");
    if (!q->last_has_cloud) return ctx_fail(ctx, UGSM_ERR_STATE, "ugsm_done_cloud: the last pair ugsm_next_done reported carried no managed cloud");
    *out = q->last_cloud;
    return UGSM_OK;
}

int ugsm_flush(ugsm_ctx *ctx)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    return no_throw(ctx, "ugsm_flush: out of host memory", [&]() -> int {
        Queue *q = queue_of(ctx);
        if (!q) return ctx_fail(ctx, UGSM_ERR_NOMEM, "ugsm_flush: out of host memory");
        q->flush_upto = q->seq;
        q->round_restarts = true;
        pump(ctx, q, false);
        return UGSM_OK;
    });
}

int ugsm_next_done(ugsm_ctx *ctx, ugsm_completion *out, int block)
{
    if (!ctx || !out) return UGSM_ERR_BAD_ARG;
    return no_throw(ctx, "ugsm_next_done: out of host memory", [&]() -> int { return next_done(ctx, out, block); });
}

int ugsm_queue_depth(ugsm_ctx *ctx, int *waiting, int *in_flight, int *unreported)
{
    if (!ctx) return UGSM_ERR_BAD_ARG;
    Queue *q = queue_of(ctx);
    if (!q) return ctx_fail(ctx, UGSM_ERR_NOMEM, "ugsm_queue_depth: out of host memory");
    int fl = 0;
    for (const Call &c : q->flight) fl += (int)c.items.size();
    if (waiting) *waiting = (int)q->waiting.size();
    if (in_flight) *in_flight = fl;
    if (unreported) *unreported = (int)q->done.size();
    return UGSM_OK;
}

}  // extern "C"
