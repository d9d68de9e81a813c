// vk_alloc_hook.hpp -- the counter behind vk_debug_set_param(ctx, "alloc_fail_at", k): which of a context's allocations is made to fail
// (vk_ctx.hpp: ctx_alloc, ctx_alloc_host).  Host only, no HIP: tests/test_alloc_failure_cpu.py compiles it on its own.
#pragma once

#include <cstdint>

namespace vk {

struct AllocFailHook {
    uint32_t at = 0;    // the allocation that fails, counted from the arming; 0: disarmed
    uint32_t seen = 0;  // allocations since the arming
    // k >= 1: the k-th allocation from now on fails; 0 disarms.  Arming again restarts the count.
    void arm(uint32_t k) { at = k; seen = 0; }
    bool armed() const { return at != 0; }
    // one allocation is about to be made: whether it is the one that fails.  The hook disarms itself when it fires.
    bool fires() {
        if (at == 0) return false;
        if (++seen < at) return false;
        at = 0; seen = 0;
        return true;
    }
};

}  // namespace vk
