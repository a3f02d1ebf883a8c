// fake_runtime_cloud.cpp -- TEST INFRASTRUCTURE: tests/fake_runtime.cpp (included whole: the same recorder, the same allocation faults) plus the
// two hooks through which csrc/ugsm_queue.cpp reaches the runtime's cloud work (CtxHooks::cloud_submit / cloud_finish, csrc/ugsm_internal.hpp),
// recorded.  A cloud submit is noted like any other call, with its spec and what kind it was; the finish hook checks that the slot had been
// seen idle, "reads the counts" -- pair b's count is the 32-bit word at the start of its left image (the test writes the pair's tag there) plus
// 100 --, asks the queue for staging of min(count, max_points) records, writes the tag into it and makes the slot busy again for the set
// number of polls.  Chosen finish calls fail with a chosen status.  Built by tests/test_queue_cloud_host.py; never shipped.
#include "fake_runtime.cpp"

#include <algorithm>

struct FakeCloud {
    long long call;  // index into ugsm_ctx::calls
    int fovea, managed, n, finishes, step;
    ugsm_queue_cloud spec;
    const uint8_t *L[UGSM_MAX_BATCH];
    CloudJob job[UGSM_MAX_BATCH];  // as handed over (W, H, stride and the format in force are in the call's own record: ugsm_fake_call_args)
};
struct FakeCloudState {
    ugsm_ctx *ctx;
    std::vector<FakeCloud> clouds;
    std::vector<int> fail_finish;  // status the finish of call k returns (0 = none)
};
static std::vector<FakeCloudState *> g_cloud_states;
static FakeCloudState *state_of(const ugsm_ctx *ctx)
{
    for (FakeCloudState *s : g_cloud_states)
        if (s->ctx == ctx) return s;
    return nullptr;
}

static int fake_cloud_submit(ugsm_ctx *ctx, int slot, const CloudCall *call)
{
    FakeCloudState *fs = state_of(ctx);
    const uint8_t *L[UGSM_MAX_BATCH], *R[UGSM_MAX_BATCH];
    int ox[UGSM_MAX_BATCH], oy[UGSM_MAX_BATCH];
    float *out[UGSM_MAX_BATCH];
    FakeCloud fc{};
    fc.call = (long long)ctx->calls.size();
    fc.fovea = call->fovea;
    fc.managed = call->managed;
    fc.n = call->n;
    fc.step = call->spec->params.format == UGSM_CLOUD_PCL32 ? 32 : 16;
    fc.spec = *call->spec;
    for (int b = 0; b < call->n; b++) {
        const CloudJob &j = fc.job[b] = call->job[b];
        fc.L[b] = L[b] = j.L;
        R[b] = j.R;
        ox[b] = j.off_x;
        oy[b] = j.off_y;
        out[b] = call->managed ? j.planes[0] : j.out;
    }
    fs->clouds.push_back(fc);  // (may throw, like the recorder's own push_back: the runtime ran out of memory before anything ran)
    const int st = submit(ctx, slot, SubmitArgs{E_CLOUD | (call->fovea ? E_FOVEA : 0) | (call->managed ? E_HOST : 0), call->n, call->W, call->H, call->stride,
                                                L, R, ox, oy, {out, nullptr, nullptr, nullptr, nullptr}});
    if (ctx->calls.size() != (size_t)fc.call + 1) fs->clouds.pop_back();
    return st;
}

static int fake_cloud_finish(ugsm_ctx *ctx, int slot, int n, ugsm_cloud_result *res, void *(*staging)(void *, int, long long), void *user)
{
    FakeCloudState *fs = state_of(ctx);
    if (slot < 0 || slot >= (int)ctx->slots.size()) return UGSM_ERR_BAD_ARG;
    FakeSlot &s = ctx->slots[(size_t)slot];
    FakeCloud *fc = nullptr;
    for (FakeCloud &c : fs->clouds)
        if (c.call == s.call) fc = &c;
    // the finish step belongs to a managed cloud call whose slot has been seen idle, and runs once, inside the queue's own calling
    if (!fc || !fc->managed || fc->n != n || s.busy || !ctx->hooks.queue_calling || fc->finishes != 0) {
        ctx->violations++;
        return UGSM_ERR_STATE;
    }
    fc->finishes++;
    const int fail = (size_t)fc->call < fs->fail_finish.size() ? fs->fail_finish[(size_t)fc->call] : 0;
    for (int b = 0; b < n && !fail; b++) {
        unsigned tag;
        memcpy(&tag, fc->L[b], sizeof tag);
        res[b] = ugsm_cloud_result{};
        res[b].count = (long long)tag + 100;
        res[b].stored = fc->spec.max_points > 0 ? std::min(res[b].count, fc->spec.max_points) : res[b].count;
        res[b].point_step = fc->step;
        res[b].levels = fc->fovea ? ctx->cfg.fovea_levels : 0;
        for (int l = 0; l < res[b].levels; l++) res[b].level_counts[l] = tag + l;
        res[b].points = staging(user, b, res[b].stored * fc->step);
        if (!res[b].points) {
            s.busy = true;  // (copies of the pairs before this one are on the stream)
            s.polls_left = ctx->poll_delay;
            ctx->calls[(size_t)s.call].drained = 0;
            return ctx_fail(ctx, UGSM_ERR_NOMEM, "fake: no staging for a pair's cloud");
        }
        memcpy(res[b].points, &tag, sizeof tag);
    }
    s.busy = true;  // the copies are on the slot's stream: busy until they have drained
    s.polls_left = ctx->poll_delay;
    ctx->calls[(size_t)s.call].drained = 0;
    if (fail) return ctx_fail(ctx, fail, "fake: this finish was told to fail");
    return UGSM_OK;
}

extern "C" {
#pragma GCC visibility push(default)
ugsm_ctx *ugsm_fake_create_cloud(int slots, int batch, int levels, int fovea_levels, int with_hooks)
{
    ugsm_ctx *c = ugsm_fake_create(slots, batch, levels, fovea_levels);
    if (!c) return nullptr;
    FakeCloudState *fs = new (std::nothrow) FakeCloudState();
    if (!fs) {
        ugsm_fake_destroy(c);
        return nullptr;
    }
    fs->ctx = c;
    fs->clouds.reserve(4096);
    g_cloud_states.push_back(fs);
    if (with_hooks) {
        c->hooks.cloud_submit = fake_cloud_submit;
        c->hooks.cloud_finish = fake_cloud_finish;
    }
    return c;
}
void ugsm_fake_destroy_cloud(ugsm_ctx *c)
{
    g_countdown = -1;
    for (size_t k = 0; k < g_cloud_states.size(); k++)
        if (g_cloud_states[k]->ctx == c) {
            delete g_cloud_states[k];
            g_cloud_states.erase(g_cloud_states.begin() + (long)k);
            break;
        }
    ugsm_fake_destroy(c);
}
int ugsm_fake_fail_finish(ugsm_ctx *c, long long index, int status)
{
    FakeCloudState *fs = state_of(c);
    if (!fs || index < 0 || index > 1 << 20) return -1;
    if (fs->fail_finish.size() <= (size_t)index) fs->fail_finish.resize((size_t)index + 1, 0);
    fs->fail_finish[(size_t)index] = status;
    return 0;
}
// call k as a cloud call: fovea, managed, pairs, times its finish hook ran, want_planes, sampling, format, compact; P1[0]; -1 if call k
// was no cloud call
int ugsm_fake_cloud_call(const ugsm_ctx *c, long long k, int *out8, double *p1_0)
{
    const FakeCloudState *fs = state_of(c);
    if (!fs) return -1;
    for (const FakeCloud &f : fs->clouds)
        if (f.call == k) {
            const int v[8] = {f.fovea, f.managed, f.n, f.finishes, f.spec.want_planes, f.spec.params.sampling, f.spec.params.format, f.spec.params.compact};
            memcpy(out8, v, sizeof v);
            *p1_0 = f.spec.P1[0];
            return 0;
        }
    return -1;
}
// the CloudJob of every pair of cloud call k, twelve words per pair: L, R, off_x, off_y, out, planes[0 .. 2], points, cap, count, level_counts;
// *reserved: the recorded spec's `reserved`; -1 if call k was no cloud call
int ugsm_fake_cloud_jobs(const ugsm_ctx *c, long long k, long long *jobs, int *reserved)
{
    const FakeCloudState *fs = state_of(c);
    if (!fs) return -1;
    for (const FakeCloud &f : fs->clouds)
        if (f.call == k) {
            for (int b = 0; b < f.n; b++) {
                const CloudJob &j = f.job[b];
                const void *p[] = {j.L, j.R, nullptr, nullptr, j.out, j.planes[0], j.planes[1], j.planes[2], j.points, nullptr, j.count, j.level_counts};
                for (int i = 0; i < 12; i++) jobs[12 * b + i] = (long long)(uintptr_t)p[i];
                jobs[12 * b + 2] = j.off_x;
                jobs[12 * b + 3] = j.off_y;
                jobs[12 * b + 9] = j.cap;
            }
            *reserved = f.spec.reserved;
            return 0;
        }
    return -1;
}
#pragma GCC visibility pop
}  // extern "C"
