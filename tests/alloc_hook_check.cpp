// The counter behind vk_debug_set_param(ctx, "alloc_fail_at", k) (vokselis_amd/csrc/vk_alloc_hook.hpp), on the CPU: armed at k it lets
// k - 1 allocations pass, fails the k-th, and is disarmed from then on; 0 disarms; arming again restarts the count.
#include "vk_alloc_hook.hpp"

#include <cstdio>

static int bad = 0;
#define HOLD(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); bad++; } } while (0)

int main() {
    unsigned long long cases = 0;
    {   // never armed: nothing fails
        vk::AllocFailHook h;
        HOLD(!h.armed());
        for (int i = 0; i < 200; i++) HOLD(!h.fires());
    }
    for (uint32_t k = 1; k <= 70; k++) {
        vk::AllocFailHook h;
        h.arm(k);
        HOLD(h.armed());
        for (uint32_t i = 1; i <= 3 * k + 5; i++, cases++) {
            const bool f = h.fires();
            HOLD(f == (i == k));            // exactly the k-th, once
            HOLD(h.armed() == (i < k));     // ... and disarmed by it
        }
        // armed again in the middle of a count: the count restarts
        for (uint32_t seen = 0; seen < k; seen++) {
            h.arm(k);
            for (uint32_t i = 0; i < seen; i++) HOLD(!h.fires());
            h.arm(k);
            for (uint32_t i = 1; i <= k; i++, cases++) HOLD(h.fires() == (i == k));
            HOLD(!h.armed());
        }
        // 0 disarms an armed hook, whatever it had counted
        for (uint32_t seen = 0; seen < k; seen++) {
            h.arm(k);
            for (uint32_t i = 0; i < seen; i++) HOLD(!h.fires());
            h.arm(0);
            HOLD(!h.armed());
            for (uint32_t i = 0; i < 2 * k; i++, cases++) HOLD(!h.fires());
        }
    }
    {   // the largest k: no wrap on the way there is asked of 2^32 calls; the count it starts from is 0
        vk::AllocFailHook h;
        h.arm(0xffffffffu);
        for (int i = 0; i < 1000; i++) HOLD(!h.fires());
        HOLD(h.armed() && h.seen == 1000u);
    }
    std::printf("hook: %llu calls\n%s\n", cases, bad ? "FAILED" : "OK");
    return bad ? 1 : 0;
}
