// fake_runtime_checked.cpp -- TEST INFRASTRUCTURE: tests/fake_runtime_cloud.cpp (included whole: the recorder, the allocation faults, the cloud
// hooks) plus the two hooks through which csrc/ugsm_queue.cpp reaches the runtime's checked full-mode call (CtxHooks::checked_submit /
// checked_marked, csrc/ugsm_internal.hpp), recorded.  A checked submit is noted like any other call (entry E_CHECKED, + E_HOST for a managed
// call, + E_CLOUD for pairs that carry a cloud), with its tau, its spec and every CheckedJob as handed over; a managed checked cloud call is
// also entered in the cloud recorder, so that the cloud fake's finish hook serves its second step.  The marked counts of pair b of a call are
// made from the 32-bit word at the start of its left image where that is real memory (a managed pair: the test writes the pair's tag there),
// else from the address: forward = word + 1000, backward = word + 2000.  The counts hook checks that the slot holds a checked call that
// has been seen drained.  Built by tests/test_queue_checked_host.py; never shipped.
#include "fake_runtime_cloud.cpp"

enum { E_CHECKED = 16 };

struct FakeChecked {
    long long call;  // index into ugsm_ctx::calls
    int managed, n, has_spec, marks;  // marks: times the counts hook ran for the call
    float tau;
    ugsm_queue_cloud spec;
    CheckedJob job[UGSM_MAX_BATCH];
    unsigned word[UGSM_MAX_BATCH];  // what the counts are made from
};
struct FakeCheckedState {
    ugsm_ctx *ctx;
    std::vector<FakeChecked> calls;
};
static std::vector<FakeCheckedState *> g_checked_states;
static FakeCheckedState *checked_state_of(const ugsm_ctx *ctx)
{
    for (FakeCheckedState *s : g_checked_states)
        if (s->ctx == ctx) return s;
    return nullptr;
}

static int fake_checked_submit(ugsm_ctx *ctx, int slot, const CheckedCall *call)
{
    FakeCheckedState *ks = checked_state_of(ctx);
    FakeCloudState *fs = state_of(ctx);
    const uint8_t *L[UGSM_MAX_BATCH], *R[UGSM_MAX_BATCH];
    float *out[3][UGSM_MAX_BATCH];
    FakeChecked fk{};
    fk.call = (long long)ctx->calls.size();
    fk.managed = call->managed;
    fk.n = call->n;
    fk.tau = call->tau;
    fk.has_spec = call->spec != nullptr;
    if (call->spec) fk.spec = *call->spec;
    FakeCloud fc{};  // (a managed checked cloud call: what the cloud fake's finish hook looks up)
    fc.call = fk.call;
    fc.managed = call->managed;
    fc.n = call->n;
    if (call->spec) {
        fc.step = call->spec->params.format == UGSM_CLOUD_PCL32 ? 32 : 16;
        fc.spec = *call->spec;
    }
    for (int b = 0; b < call->n; b++) {
        const CheckedJob &j = fk.job[b] = call->job[b];
        fc.L[b] = L[b] = j.L;
        R[b] = j.R;
        if (call->managed) memcpy(&fk.word[b], j.L, sizeof(unsigned));
        else fk.word[b] = (unsigned)((uintptr_t)j.L >> 12);
        for (int k = 0; k < 3; k++) out[k][b] = call->managed ? j.planes[k] : (k == 0 ? j.out : nullptr);
    }
    const bool second_step = call->spec && call->managed;
    ks->calls.push_back(fk);  // (may throw, like the recorder's own push_back: the runtime ran out of memory before anything ran)
    if (second_step) {
        try {
            fs->clouds.push_back(fc);
        } catch (...) {
            ks->calls.pop_back();
            throw;
        }
    }
    const int entry = E_CHECKED | (call->managed ? E_HOST : 0) | (call->spec ? E_CLOUD : 0);
    int st;
    try {
        st = submit(ctx, slot, SubmitArgs{entry, call->n, call->W, call->H, call->stride, L, R, nullptr, nullptr, {out[0], out[1], out[2], nullptr, nullptr}});
    } catch (...) {
        ks->calls.pop_back();
        if (second_step) fs->clouds.pop_back();
        throw;
    }
    if (ctx->calls.size() != (size_t)fk.call + 1) {  // (refused by the recorder: no call)
        ks->calls.pop_back();
        if (second_step) fs->clouds.pop_back();
    }
    return st;
}

static int fake_checked_marked(ugsm_ctx *ctx, int slot, int n, long long *fwd, long long *back)
{
    FakeCheckedState *ks = checked_state_of(ctx);
    if (slot < 0 || slot >= (int)ctx->slots.size()) return UGSM_ERR_BAD_ARG;
    FakeSlot &s = ctx->slots[(size_t)slot];
    FakeChecked *fk = nullptr;
    for (FakeChecked &c : ks->calls)
        if (c.call == s.call) fk = &c;
    // the counts belong to the checked call the slot still holds, are read once, and only when the slot has been seen drained
    if (!fk || fk->n != n || s.busy || fk->marks != 0 || !ctx->calls[(size_t)s.call].drained) {
        ctx->violations++;
        return UGSM_ERR_STATE;
    }
    fk->marks++;
    for (int b = 0; b < n; b++) {
        fwd[b] = (long long)fk->word[b] + 1000;
        back[b] = (long long)fk->word[b] + 2000;
    }
    return UGSM_OK;
}

extern "C" {
#pragma GCC visibility push(default)
// hooks: bit 0 the cloud hooks, bit 1 the checked hooks
ugsm_ctx *ugsm_fake_create_checked(int slots, int batch, int levels, int fovea_levels, int hooks)
{
    ugsm_ctx *c = ugsm_fake_create_cloud(slots, batch, levels, fovea_levels, hooks & 1);
    if (!c) return nullptr;
    FakeCheckedState *ks = new (std::nothrow) FakeCheckedState();
    if (!ks) {
        ugsm_fake_destroy_cloud(c);
        return nullptr;
    }
    ks->ctx = c;
    ks->calls.reserve(4096);
    g_checked_states.push_back(ks);
    if (hooks & 2) {
        c->hooks.checked_submit = fake_checked_submit;
        c->hooks.checked_marked = fake_checked_marked;
    }
    return c;
}
void ugsm_fake_destroy_checked(ugsm_ctx *c)
{
    g_countdown = -1;
    for (size_t k = 0; k < g_checked_states.size(); k++)
        if (g_checked_states[k]->ctx == c) {
            delete g_checked_states[k];
            g_checked_states.erase(g_checked_states.begin() + (long)k);
            break;
        }
    ugsm_fake_destroy_cloud(c);
}
// the context's configuration words a checked pair is refused for
void ugsm_fake_set_config(ugsm_ctx *c, float early_exit_threshold, int kernel_path)
{
    c->cfg.early_exit_threshold = early_exit_threshold;
    c->cfg.kernel_path = kernel_path;
}
// call k as a checked call: managed, pairs, whether it came with a spec, times the counts hook ran, the spec's want_planes and compact; *tau: its
// threshold, bit for bit; -1 if call k was no checked call
int ugsm_fake_checked_call(const ugsm_ctx *c, long long k, int *out6, float *tau)
{
    const FakeCheckedState *ks = checked_state_of(c);
    if (!ks) return -1;
    for (const FakeChecked &f : ks->calls)
        if (f.call == k) {
            const int v[6] = {f.managed, f.n, f.has_spec, f.marks, f.spec.want_planes, f.spec.params.compact};
            memcpy(out6, v, sizeof v);
            *tau = f.tau;
            return 0;
        }
    return -1;
}
// the CheckedJob of every pair of checked call k, thirteen words per pair: L, R, out, back, planes[0 .. 2], back_planes[0 .. 2], points, cap, count;
// *p1_0, *reserved: P1[0] and `reserved` of the recorded spec; -1 if call k was no checked call
int ugsm_fake_checked_jobs(const ugsm_ctx *c, long long k, long long *jobs, double *p1_0, int *reserved)
{
    const FakeCheckedState *ks = checked_state_of(c);
    if (!ks) return -1;
    for (const FakeChecked &f : ks->calls)
        if (f.call == k) {
            for (int b = 0; b < f.n; b++) {
                const CheckedJob &j = f.job[b];
                const void *p[] = {j.L, j.R, j.out, j.back, j.planes[0], j.planes[1], j.planes[2], j.back_planes[0], j.back_planes[1], j.back_planes[2],
                                   j.points, nullptr, j.count};
                for (int i = 0; i < 13; i++) jobs[13 * b + i] = (long long)(uintptr_t)p[i];
                jobs[13 * b + 11] = j.cap;
            }
            *p1_0 = f.spec.P1[0];
            *reserved = f.spec.reserved;
            return 0;
        }
    return -1;
}
#pragma GCC visibility pop
}  // extern "C"
