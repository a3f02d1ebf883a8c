// ugsm_mem.hpp -- the memory a slot's calls run on, as types that hold the rules: a device buffer with its capacity (DevBuf), the one capacity
// of several that grow together (GroupCap), a page-locked buffer (PinnedBuf), a device table with the page-locked copies it goes up from
// (UploadRing), and the context's accounting of it all (MemBook).  Host only: the HIP runtime API and the standard library, nothing of the
// project -- tests/slot_mem_sanitize.cpp compiles it with g++ against stand-ins for the runtime.
// A context here is anything with a `MemBook book` and a `std::string err`.  No type frees in a destructor: release() is explicit, because
// freeing needs the device set and the streams drained, which ugsm_destroy decides.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <string>

namespace ugsm {

constexpr int kMemOk = 0, kMemErrDevice = 5, kMemErrNoMem = 6;  // UGSM_OK, UGSM_ERR_DEVICE, UGSM_ERR_NOMEM (include/ugsm.h; ugsm_slot.hpp asserts it)

struct MemBook {
    long long dev_bytes = 0;    // device memory held by the counted buffers (each knows its own share); ugsm_context_device_bytes
    long long release_epoch = 0;  // counts the releases of counted buffers: "memory may have come free since" (prepare_slot)
    long long mem_limit = 0;    // development (UGSM_MEM_LIMIT_MB under UGSM_DEV=1): counted buffers do not grow past it -- the UGSM_ERR_NOMEM path without exhausting a GPU
    void untrack(size_t bytes)
    {
        dev_bytes -= (long long)bytes;
        release_epoch++;
    }
};

#define HIPCHK(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess) {                                                                      \
            char b__[512];                                                                            \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            (ctx)->err = b__;                                                                         \
            return ::ugsm::kMemErrDevice;                                                             \
        }                                                                                             \
    } while (0)

// A device buffer and its capacity (elements).  Reads as its pointer.  Counted: in the context's book and under its limit.
template <class T, bool Counted = true>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    operator T *() const { return p; }
    // room for `need` elements; what the buffer held is not kept.  The old buffer goes first -- the two are never held together -- and a
    // failure leaves none.
    template <class Ctx>
    int grow(Ctx *ctx, size_t need)
    {
        if (need <= cap) return kMemOk;  // (every call of the submit path comes through here)
        T *const old = p;
        if (Counted && old) ctx->book.untrack(cap * sizeof(T));
        p = nullptr;
        cap = 0;
        if (old) HIPCHK(ctx, hipFree(old));
        const size_t bytes = need * sizeof(T);
        const bool over = Counted && ctx->book.mem_limit > 0 && ctx->book.dev_bytes + (long long)bytes > ctx->book.mem_limit;
        const hipError_t e = over ? hipErrorOutOfMemory : hipMalloc((void **)&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();  // (the failed allocation must not poison the next launch check)
            char b[256];
            snprintf(b, sizeof b, "hipMalloc of %zu bytes failed: %s (the context holds %lld bytes)", bytes, hipGetErrorString(e), ctx->book.dev_bytes);
            ctx->err = b;
            p = nullptr;  // (whatever the failed call left there)
            return kMemErrNoMem;
        }
        cap = need;
        if (Counted) ctx->book.dev_bytes += (long long)bytes;
        return kMemOk;
    }
    template <class Ctx>
    void release(Ctx *ctx)
    {
        if (p) {
            if (Counted) ctx->book.untrack(cap * sizeof(T));
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
    }
};

// The one capacity of several DevBufs that grow together, in the order given: every member holds `cap` elements, or -- after a failure
// part-way -- none holds anything and the capacity is 0, never a capacity that some member lacks.
struct GroupCap {
    size_t cap = 0;
    operator size_t() const { return cap; }
    template <class Ctx, class T>
    int grow(Ctx *ctx, size_t need, std::initializer_list<DevBuf<T> *> members)
    {
        if (need <= cap) return kMemOk;
        cap = 0;
        for (DevBuf<T> *m : members)
            if (int st = m->grow(ctx, need)) {
                release(ctx, members);
                return st;
            }
        cap = need;
        return kMemOk;
    }
    template <class Ctx, class T>
    void release(Ctx *ctx, std::initializer_list<DevBuf<T> *> members)
    {
        for (DevBuf<T> *m : members) m->release(ctx);
        cap = 0;
    }
};

// Page-locked host memory and its capacity (elements).  Not counted.
template <class T>
struct PinnedBuf {
    T *p = nullptr;
    size_t cap = 0;
    operator T *() const { return p; }
    template <class Ctx>
    int grow(Ctx *ctx, size_t need)
    {
        if (need <= cap) return kMemOk;
        if (p) HIPCHK(ctx, hipHostFree(p));
        p = nullptr;
        cap = 0;
        HIPCHK(ctx, hipHostMalloc((void **)&p, need * sizeof(T), hipHostMallocDefault));
        cap = need;
        return kMemOk;
    }
    template <class Ctx>
    void release(Ctx *)
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

inline void destroy_event(hipEvent_t &e)
{
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
}

// release(ctx) of every one of them
template <class Ctx, class... Bufs>
void release_all(Ctx *ctx, Bufs &...bufs)
{
    (bufs.release(ctx), ...);
}

// A table of rows in device memory and the page-locked copies it is uploaded from on a stream.  The caller does not wait for the stream, so a
// copy may still be read by an earlier call's upload when the next call fills its rows: N copies take turns, each with an event behind its
// upload, and a call waits only for the UPLOAD of the call N before it.  Growing waits for the stream -- an earlier call's kernels may still
// read the table, its upload the copies -- and forgets the uploads recorded.
template <class Row, int N = 4>
struct UploadRing {
    DevBuf<Row> tab;
    PinnedBuf<Row> copies;  // N x (copies.cap / N) rows
    hipEvent_t ev[N] = {};
    bool recorded[N] = {};
    int next = 0, turn = 0;
    // the rows of this call's turn, to be filled: room for `rows` of them
    template <class Ctx>
    int begin(Ctx *ctx, hipStream_t st, size_t rows, Row **out)
    {
        if (rows > tab.cap || N * rows > copies.cap) {
            HIPCHK(ctx, hipStreamSynchronize(st));
            if (int r = tab.grow(ctx, rows)) return r;
            if (int r = copies.grow(ctx, N * rows)) return r;
            for (bool &set : recorded) set = false;
        }
        turn = next;
        next = (turn + 1) % N;
        if (!ev[turn]) HIPCHK(ctx, hipEventCreateWithFlags(&ev[turn], hipEventDisableTiming));
        if (recorded[turn]) HIPCHK(ctx, hipEventSynchronize(ev[turn]));  // (the upload of the call N back: long done)
        *out = copies + (size_t)turn * (copies.cap / N);
        return kMemOk;
    }
    // the first n rows of this turn into the table
    template <class Ctx>
    int upload(Ctx *ctx, hipStream_t st, size_t n)
    {
        HIPCHK(ctx, hipMemcpyAsync(tab, copies + (size_t)turn * (copies.cap / N), n * sizeof(Row), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipEventRecord(ev[turn], st));
        recorded[turn] = true;
        return kMemOk;
    }
    template <class Ctx>
    void release(Ctx *ctx)
    {
        release_all(ctx, tab, copies);
        for (hipEvent_t &e : ev) destroy_event(e);
        *this = UploadRing{};
    }
};

}  // namespace ugsm
