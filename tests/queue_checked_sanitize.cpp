// queue_checked_sanitize.cpp -- TEST INFRASTRUCTURE: a program of its own (main below) made of csrc/ugsm_queue.cpp and the three fakes
// (tests/fake_runtime_checked.cpp includes the other two), for a build with -fsanitize=address,undefined on the CPU: about sixty mixed pairs
// -- plain, managed, cloud and the four checked kinds, taus that change, back fields taken and not -- through the queue, every completion
// fetched, the lent planes written to; then the same burst once more under every single host allocation failure.  Prints what it did; exits
// non-zero when a pair is lost, reported twice or out of order.  Built and run by tests/test_queue_checked_host.py; never shipped.
#include "fake_runtime_checked.cpp"

#include <cstdio>

static int burst(ugsm_ctx *ctx, std::vector<uint64_t> &accepted, std::vector<uint64_t> &reported, long long *failed_pairs)
{
    static uint8_t img[2][16 * 3 * 32];
    uint8_t *const dev = reinterpret_cast<uint8_t *>(0x7F0000000000ull);  // made-up device addresses: never looked behind
    ugsm_queue_cloud spec{};
    spec.P1[0] = spec.P2[0] = 1.0;
    spec.params.sampling = 1;
    spec.params.z_min = -1e30f;
    spec.params.z_max = 1e30f;
    spec.want_planes = 1;
    auto fetch = [&](int block, bool all) {
        ugsm_completion c;
        for (int spins = 0; spins < 100; spins++) {
            const int st = ugsm_next_done(ctx, &c, block);
            if (st == UGSM_ERR_NOMEM) continue;  // (an allocation fault inside the fetch: nothing was consumed)
            if (st != UGSM_OK) return;
            reported.push_back(c.tag);
            if (c.status != UGSM_OK) ++*failed_pairs;
            for (int k = 0; k < 3; k++)
                if (c.result[k]) c.result[k][0] = c.result[k][32 * 16 - 1] = 1.0f;  // the lent planes are the host's to touch
            ugsm_checked_result r;
            if (ugsm_done_checked(ctx, &r) == UGSM_OK)
                for (int k = 0; k < 3; k++)
                    if (r.back[k]) r.back[k][0] = r.back[k][32 * 16 - 1] = 2.0f;
            ugsm_cloud_result cr;
            if (ugsm_done_cloud(ctx, &cr) == UGSM_OK && cr.stored > 0) static_cast<char *>(cr.points)[cr.stored * cr.point_step - 1] = 1;
            if (!all) return;
        }
    };
    for (int k = 0; k < 62; k++) {
        const uint64_t tag = accepted.size();
        const unsigned word = (unsigned)tag;
        memcpy(img[0], &word, sizeof word);
        uint8_t *const p = dev + 4096 * tag;
        float *const out = reinterpret_cast<float *>(p + 256), *const back = (k & 1) ? reinterpret_cast<float *>(p + 512) : nullptr;
        long long *const count = reinterpret_cast<long long *>(p + 1024);
        const float tau = (k / 9) & 1 ? 0.5f : 1.0f;
        auto enqueue = [&]() -> int {
            switch (k % 7) {
            case 0: return ugsm_enqueue_full_checked(ctx, p, p + 64, 64, 32, 192, out, back, tau, tag);
            case 1: return ugsm_enqueue_full_checked_managed(ctx, img[0], img[1], 32, 16, 96, tau, k & 2, tag);
            case 2: return ugsm_enqueue_full_checked_cloud(ctx, p, p + 64, 64, 32, 192, out, back, tau, &spec, p + 2048, 100, count, tag);
            case 3: return ugsm_enqueue_full_checked_cloud_managed(ctx, img[0], img[1], 32, 16, 96, tau, k & 2, &spec, tag);
            case 4: return ugsm_enqueue_full(ctx, p, p + 64, 64, 32, 192, out, tag);
            case 5: return ugsm_enqueue_full_managed(ctx, img[0], img[1], 32, 16, 96, tag);
            default: return ugsm_enqueue_full_cloud_managed(ctx, img[0], img[1], 32, 16, 96, &spec, tag);
            }
        };
        int st = enqueue();
        if (st == UGSM_ERR_STATE) {  // (a full queue: fetch the oldest pair, then once more)
            fetch(1, false);
            st = enqueue();
        }
        if (st == UGSM_OK) accepted.push_back(tag);
        else if (st != UGSM_ERR_NOMEM) return 1;
        if (k % 3 == 2) fetch(0, false);
    }
    (void)ugsm_flush(ctx);
    fetch(1, true);
    return 0;
}

int main()
{
    long long pairs = 0, failed_pairs = 0, runs = 0, refused_runs = 0;
    const long long a0 = g_allocs;
    long long n_allocs = 0;
    for (long long fault = -1; fault <= n_allocs + 1; fault++, runs++) {
        ugsm_ctx *ctx = ugsm_fake_create_checked(2, 3, 8, 4, 3);
        if (!ctx) return 2;
        ugsm_fake_poll_delay(ctx, 1);
        std::vector<uint64_t> accepted, reported;
        accepted.reserve(256);
        reported.reserve(256);
        const long long before = g_allocs;
        ugsm_fake_fail_alloc_after(fault);
        const int st = burst(ctx, accepted, reported, &failed_pairs);
        ugsm_fake_fail_alloc_after(-1);
        if (fault < 0) n_allocs = g_allocs - before;
        if (st != 0 || accepted != reported || ctx->violations != 0) {
            fprintf(stderr, "fault %lld: status %d, %zu accepted, %zu reported, %d violations\n", fault, st, accepted.size(), reported.size(), ctx->violations);
            return 1;
        }
        if (fault < 0 && accepted.size() != 62) return 3;
        refused_runs += accepted.size() < 62;
        pairs += (long long)accepted.size();
        // the queue is usable afterwards: the same burst again, nothing failing
        std::vector<uint64_t> again = accepted, again_reported = reported;
        again.reserve(512);
        again_reported.reserve(512);
        long long failed_again = 0;
        if (burst(ctx, again, again_reported, &failed_again) != 0 || again != again_reported || again.size() != accepted.size() + 62 || failed_again != 0) return 4;
        pairs += 62;
        ugsm_fake_destroy_checked(ctx);
    }
    printf("ok: %lld runs of 62 mixed pairs (%lld host allocations in the first, %lld since start), one failing allocation each in %lld of them: %lld pairs "
           "accepted, each reported once and in order; %lld runs saw a pair refused, %lld pairs reported with a failed call\n",
           runs, n_allocs, g_allocs - a0, runs - 1, pairs, refused_runs, failed_pairs);
    return 0;
}
