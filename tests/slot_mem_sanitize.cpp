// The slot's memory types (csrc/ugsm_mem.hpp: MemBook, DevBuf, GroupCap, PinnedBuf, UploadRing) as a program of their own, for the address
// and undefined-behaviour sanitizers on the CPU: the runtime calls the header uses are malloc-backed stand-ins that count what is live,
// can fail the k-th device allocation or refuse above a byte limit, and log every wait.  tests/test_slot_mem_host.py builds and runs it.
#include "../ug_stereomatcher_amd/csrc/ugsm_mem.hpp"

#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

// ---- the stand-ins ------------------------------------------------------------------------------------------------------------------------
namespace {
std::map<void *, size_t> g_dev, g_host;  // live allocations and their bytes
size_t g_dev_peak = 0, g_host_peak = 0;  // the most that were ever live at once (reset by the tests)
long long g_dev_mallocs = 0, g_host_mallocs = 0, g_fail_at = -1;  // g_fail_at: the device allocation of that number fails (counted from 0)
size_t g_byte_limit = 0;                 // > 0: device allocations that would take the live bytes past it fail
long long g_events = 0, g_stream_syncs = 0, g_last_error_reads = 0;
struct FakeEvent {
    bool recorded = false;
};
std::vector<hipEvent_t> g_event_waits;   // every hipEventSynchronize, in order

size_t live_bytes(const std::map<void *, size_t> &m)
{
    size_t n = 0;
    for (const auto &kv : m) n += kv.second;
    return n;
}
[[noreturn]] void fail(const char *what, int line)
{
    fprintf(stderr, "slot_mem_sanitize: line %d: %s\n", line, what);
    exit(1);
}
#define CHECK(cond)                      \
    do {                                 \
        if (!(cond)) fail(#cond, __LINE__); \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes)
{
    const long long k = g_dev_mallocs++;
    if (k == g_fail_at || (g_byte_limit && live_bytes(g_dev) + bytes > g_byte_limit)) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_dev[*p] = bytes;
    if (g_dev.size() > g_dev_peak) g_dev_peak = g_dev.size();
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    CHECK(g_dev.erase(p) == 1);  // (never a pointer that is not live: no double free, no foreign pointer)
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int)
{
    g_host_mallocs++;
    *p = malloc(bytes ? bytes : 1);
    g_host[*p] = bytes;
    if (g_host.size() > g_host_peak) g_host_peak = g_host.size();
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    CHECK(g_host.erase(p) == 1);
    free(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    *e = reinterpret_cast<hipEvent_t>(new FakeEvent);
    g_events++;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    reinterpret_cast<FakeEvent *>(e)->recorded = true;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    CHECK(reinterpret_cast<FakeEvent *>(e)->recorded);  // (nobody waits for an event that was never recorded)
    g_event_waits.push_back(e);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    delete reinterpret_cast<FakeEvent *>(e);
    g_events--;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    g_stream_syncs++;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t)
{
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    g_last_error_reads++;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some error"; }
}

// ---- the tests ----------------------------------------------------------------------------------------------------------------------------
namespace {
using namespace ugsm;

struct Ctx {
    MemBook book;
    std::string err;
};

// the book's bytes are the live device allocations' but for `uncounted` bytes
void check_book(const Ctx &c, size_t uncounted = 0) { CHECK((size_t)c.book.dev_bytes + uncounted == live_bytes(g_dev)); }

void test_single_growth()
{
    Ctx c;
    DevBuf<float> b;
    DevBuf<double, false> u;
    g_dev_peak = 0;
    CHECK(b.grow(&c, 100) == kMemOk && b.p && b.cap == 100 && (float *)b == b.p);
    check_book(c);
    CHECK(c.book.dev_bytes == 400 && c.book.release_epoch == 0);
    b.p[99] = 1.0f;  // (the sanitizer watches the room)
    long long calls = g_dev_mallocs;
    CHECK(b.grow(&c, 100) == kMemOk && b.grow(&c, 7) == kMemOk && b.grow(&c, 0) == kMemOk);  // a smaller need allocates nothing
    CHECK(g_dev_mallocs == calls && b.cap == 100 && c.book.release_epoch == 0);
    CHECK(b.grow(&c, 1000) == kMemOk && b.cap == 1000);  // a larger need frees, then allocates: never both
    CHECK(g_dev_peak == 1 && g_dev.size() == 1 && c.book.release_epoch == 1);
    check_book(c);
    b.p[999] = 2.0f;
    // an uncounted buffer never moves the book, nor the release count, and knows no limit
    const long long bytes = c.book.dev_bytes, epoch = c.book.release_epoch;
    c.book.mem_limit = 4000;
    CHECK(u.grow(&c, 50) == kMemOk && u.grow(&c, 5000) == kMemOk && u.cap == 5000);
    CHECK(c.book.dev_bytes == bytes && c.book.release_epoch == epoch);
    check_book(c, 5000 * sizeof(double));
    // the limit: refused without asking the runtime; no buffer, no capacity, the error cleared, the message, UGSM_ERR_NOMEM
    calls = g_dev_mallocs;
    const long long reads = g_last_error_reads;
    CHECK(b.grow(&c, 1001) == kMemErrNoMem && !b.p && b.cap == 0 && g_dev_mallocs == calls && g_last_error_reads == reads + 1);
    CHECK(c.err == "hipMalloc of 4004 bytes failed: out of memory (the context holds 0 bytes)");
    CHECK(c.book.dev_bytes == 0 && c.book.release_epoch == epoch + 1);  // (the old buffer went first)
    check_book(c, 5000 * sizeof(double));
    CHECK(b.grow(&c, 1000) == kMemOk && c.book.dev_bytes == 4000);  // exactly at the limit fits
    c.book.mem_limit = 0;
    // the runtime's own refusal: the same end
    g_fail_at = g_dev_mallocs;
    CHECK(b.grow(&c, 2000) == kMemErrNoMem && !b.p && b.cap == 0 && c.book.dev_bytes == 0);
    CHECK(c.err == "hipMalloc of 8000 bytes failed: out of memory (the context holds 0 bytes)");
    g_fail_at = -1;
    CHECK(b.grow(&c, 2000) == kMemOk);  // a later growth succeeds
    check_book(c, 5000 * sizeof(double));
    // releases: counted ones advance the count, every one nulls
    const long long e2 = c.book.release_epoch;
    b.release(&c);
    CHECK(!b.p && b.cap == 0 && c.book.release_epoch == e2 + 1 && c.book.dev_bytes == 0);
    b.release(&c);  // (of nothing: nothing)
    u.release(&c);
    CHECK(!u.p && u.cap == 0 && c.book.release_epoch == e2 + 1);
    CHECK(g_dev.empty());
}

void test_pinned()
{
    Ctx c;
    PinnedBuf<long long> h;
    g_host_peak = 0;
    CHECK(h.grow(&c, 3) == kMemOk && h.cap == 3);
    h.p[2] = 5;
    const long long calls = g_host_mallocs;
    CHECK(h.grow(&c, 3) == kMemOk && h.grow(&c, 1) == kMemOk && g_host_mallocs == calls);
    CHECK(h.grow(&c, 64) == kMemOk && h.cap == 64 && g_host_peak == 1 && g_host.size() == 1);
    h.p[63] = 7;
    CHECK(c.book.dev_bytes == 0);  // (not counted)
    h.release(&c);
    h.release(&c);
    CHECK(!h.p && h.cap == 0 && g_host.empty());
}

// groups of K members: every allocation at which a growth can fail, from nothing and from a group that holds something; by the k-th
// allocation failing, by the runtime's byte limit and by the book's
template <int K>
int grow_group(Ctx &c, GroupCap &cap, DevBuf<float> *m, size_t need)
{
    if (K == 2) return cap.grow(&c, need, {&m[0], &m[1]});
    if (K == 3) return cap.grow(&c, need, {&m[0], &m[1], &m[2]});
    return cap.grow(&c, need, {&m[0], &m[1], &m[2], &m[3], &m[4]});
}
template <int K>
void test_group()
{
    for (int how = 0; how < 3; how++)
        for (int grown = 0; grown < 2; grown++)
            for (int k = 0; k < K; k++) {
                Ctx c;
                DevBuf<float> other, m[5];
                GroupCap cap;
                CHECK(other.grow(&c, 10) == kMemOk);  // a bystander: what the book must come back to
                if (grown) {
                    CHECK(grow_group<K>(c, cap, m, 100) == kMemOk && cap == 100);
                    const long long calls = g_dev_mallocs;
                    CHECK(grow_group<K>(c, cap, m, 100) == kMemOk && grow_group<K>(c, cap, m, 1) == kMemOk && g_dev_mallocs == calls);
                    for (int j = 0; j < K; j++) CHECK(m[j].p && m[j].cap == 100);
                    CHECK(c.book.dev_bytes == 40 + K * 400);
                }
                const size_t need = 1000, bytes = need * sizeof(float);
                // member k's allocation fails: members 0 .. k-1 hold the new size then, the members behind k still hold the old one
                const size_t before_k = 40 + k * bytes + (grown ? (K - 1 - k) * 400 : 0);
                if (how == 0) g_fail_at = g_dev_mallocs + k;
                if (how == 1) g_byte_limit = before_k + bytes - 1;
                if (how == 2) c.book.mem_limit = (long long)(before_k + bytes - 1);
                CHECK(grow_group<K>(c, cap, m, need) == kMemErrNoMem);
                g_fail_at = -1;
                g_byte_limit = 0;
                c.book.mem_limit = 0;
                for (int j = 0; j < 5; j++) CHECK(!m[j].p && m[j].cap == 0);  // no member is held
                CHECK(cap == 0 && cap.cap == 0);
                CHECK(c.book.dev_bytes == 40 && g_dev.size() == 1);  // the book is back to the bystander's
                check_book(c);
                CHECK(c.err.rfind("hipMalloc of 4000 bytes failed: out of memory", 0) == 0);
                CHECK(grow_group<K>(c, cap, m, need) == kMemOk && cap == need);  // a later growth succeeds
                for (int j = 0; j < K; j++) {
                    CHECK(m[j].p && m[j].cap == need);
                    m[j].p[need - 1] = 1.0f;
                }
                CHECK(c.book.dev_bytes == (long long)(40 + K * bytes));
                check_book(c);
                if (K == 2) cap.release(&c, {&m[0], &m[1]});
                if (K == 3) cap.release(&c, {&m[0], &m[1], &m[2]});
                if (K == 5) cap.release(&c, {&m[0], &m[1], &m[2], &m[3], &m[4]});
                CHECK(cap == 0 && c.book.dev_bytes == 40);
                other.release(&c);
                CHECK(g_dev.empty() && c.book.dev_bytes == 0);
            }
}

struct Row {
    long long v[3];
};
void test_ring()
{
    constexpr int N = 4;
    Ctx c;
    UploadRing<Row, N> ring;
    hipStream_t st = nullptr;
    const size_t rows = 6;
    long long syncs = g_stream_syncs;
    std::vector<Row *> seen;
    g_event_waits.clear();
    for (int t = 0; t < 2 * N + 1; t++) {
        const size_t waits = g_event_waits.size();
        Row *r = nullptr;
        CHECK(ring.begin(&c, st, rows, &r) == kMemOk && r);
        if (t == 0) {  // the first turn makes the table and the copies, behind a wait for the stream
            CHECK(g_stream_syncs == syncs + 1 && ring.tab.cap == rows && ring.copies.cap == N * rows && c.book.dev_bytes == (long long)(rows * sizeof(Row)));
        }
        CHECK(g_stream_syncs == syncs + 1);
        CHECK(r == ring.copies.p + (t % N) * rows);  // the rows cycle through the N copies
        seen.push_back(r);
        // a turn waits for its own previous upload and for no other; the first N turns wait for nothing
        if (t < N) CHECK(g_event_waits.size() == waits);
        else CHECK(g_event_waits.size() == waits + 1 && g_event_waits.back() == ring.ev[t % N]);
        // upload copies exactly n rows
        const size_t n = 1 + t % rows;
        for (size_t i = 0; i < rows; i++) r[i] = Row{{t, (long long)i, 7}};
        for (size_t i = 0; i < rows; i++) ring.tab.p[i] = Row{{-1, -1, -1}};
        CHECK(ring.upload(&c, st, n) == kMemOk);
        for (size_t i = 0; i < rows; i++) {
            const Row want = i < n ? Row{{t, (long long)i, 7}} : Row{{-1, -1, -1}};
            CHECK(memcmp(&ring.tab.p[i], &want, sizeof want) == 0);
        }
    }
    for (int t = 0; t < N; t++)
        for (int u = 0; u < t; u++) CHECK(seen[t] != seen[u]);
    CHECK(seen[N] == seen[0] && seen[2 * N] == seen[0]);
    // fewer rows: nothing grows, the copies stay where they are
    {
        Row *r = nullptr;
        const long long dm = g_dev_mallocs, hm = g_host_mallocs;
        CHECK(ring.begin(&c, st, 2, &r) == kMemOk && r == ring.copies.p + ((2 * N + 1) % N) * rows && g_dev_mallocs == dm && g_host_mallocs == hm);
        CHECK(ring.upload(&c, st, 2) == kMemOk);
    }
    // a growth in the middle waits for the stream and drops the recorded uploads: the next N turns wait for nothing
    syncs = g_stream_syncs;
    const size_t more = 11;
    for (int t = 0; t < N + 1; t++) {
        const size_t waits = g_event_waits.size();
        Row *r = nullptr;
        CHECK(ring.begin(&c, st, more, &r) == kMemOk);
        CHECK(g_stream_syncs == syncs + 1 && ring.tab.cap == more && ring.copies.cap == N * more);
        CHECK(r == ring.copies.p + ring.turn * more);
        if (t < N) CHECK(g_event_waits.size() == waits);
        else CHECK(g_event_waits.size() == waits + 1 && g_event_waits.back() == ring.ev[ring.turn]);
        r[more - 1] = Row{{1, 2, 3}};
        CHECK(ring.upload(&c, st, more) == kMemOk);
    }
    CHECK(c.book.dev_bytes == (long long)(more * sizeof(Row)) && g_dev.size() == 1 && g_host.size() == 1 && g_events == N);
    check_book(c);
    // a failed growth leaves a ring that grows again
    g_fail_at = g_dev_mallocs;
    Row *r = nullptr;
    CHECK(ring.begin(&c, st, 100, &r) == kMemErrNoMem && !ring.tab.p && ring.tab.cap == 0 && c.book.dev_bytes == 0);
    g_fail_at = -1;
    CHECK(ring.begin(&c, st, 100, &r) == kMemOk && r && ring.tab.cap == 100 && ring.copies.cap == N * 100);
    r[99] = Row{{1, 1, 1}};
    CHECK(ring.upload(&c, st, 100) == kMemOk);
    ring.release(&c);
    CHECK(g_dev.empty() && g_host.empty() && g_events == 0 && c.book.dev_bytes == 0);
}

// a slot's worth of everything, used and released: nothing is left
void test_release_of_everything()
{
    Ctx c;
    DevBuf<float> a, b, l, r;
    DevBuf<unsigned, false> word;
    GroupCap ab, lr;
    PinnedBuf<double> h;
    UploadRing<Row> ring, unused;
    Row *rows = nullptr;
    CHECK(word.grow(&c, 16) == kMemOk && ab.grow(&c, 10, {&a, &b}) == kMemOk && lr.grow(&c, 20, {&l, &r}) == kMemOk && h.grow(&c, 3) == kMemOk);
    CHECK(ring.begin(&c, nullptr, 5, &rows) == kMemOk && ring.upload(&c, nullptr, 5) == kMemOk);
    check_book(c, 16 * sizeof(unsigned));
    ab.release(&c, {&a, &b});
    lr.release(&c, {&l, &r});
    word.release(&c);
    h.release(&c);
    ring.release(&c);
    unused.release(&c);
    CHECK(g_dev.empty() && g_host.empty() && g_events == 0);
    CHECK(c.book.dev_bytes == 0);
}
}  // namespace

int main()
{
    test_single_growth();
    test_pinned();
    test_group<2>();
    test_group<3>();
    test_group<5>();
    test_ring();
    test_release_of_everything();
    CHECK(g_dev.empty() && g_host.empty() && g_events == 0);
    printf("ok: %lld device allocations, %lld page-locked\n", g_dev_mallocs, g_host_mallocs);
    return 0;
}
