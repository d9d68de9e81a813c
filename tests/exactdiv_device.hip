// exactdiv_device.hip -- the helpers of vokselis_amd/csrc/vk_exactdiv.hpp against the plain `/` expressions they replace in the cell march's ray
// set-up, ON THE DEVICE: the division the compiler expands (v_div_scale_f32 / v_rcp_f32 / v_div_fmas_f32 / v_div_fixup_f32) is the reference.
// A stand-alone program (tests/test_ray_setup_gpu.py builds it with hipcc, the product's flags, and runs it once as a child process).
//
//   chain   every mantissa of the divisor b x exponents -40 .. 40 in steps of 8, either sign (by the mantissa's parity); numerators 1 and a hashed
//           in-range value: div_inrange(a, b), div_by(a, recip_refine(b)) and div_inrange(1, b) against a / b and 1 / b
//   const   div_const(2 (x + 0.5), W, RN(1 / W) from the host) against (2 (x + 0.5)) / W for every x < W <= 8192
//   dt      every mantissa of d (in [0.5, 1) and in [2^-21, 2^-20), either sign) x fn = 2^3 .. 2^11: |div_inrange(1, d)| pow2_recip(fn), and the same
//           from the generic 1 / d, against 1 / (fn |d|)
// Prints one line per part, "<part>: <cases> cases, <n> differences", then what v_rcp_f32 makes of the host's one seed-dependent case
// (tests/exactdiv_fuzz.cpp), 1 / 0x1.fffffep0.  Exit code 0 when it ran; the differences are the caller's to judge.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "vk_exactdiv.hpp"

using namespace vk;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)

struct Result {
    unsigned long long diff[3];   // chain, const, dt
    unsigned long long cases[3];
    uint32_t first[3][4];         // the first difference of each part: operands and both results, as bits
    float rcp_allones, div_allones, chain_allones;
};

__device__ __forceinline__ uint32_t bits(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float from_bits(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t hash32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

__device__ __forceinline__ void report(Result *R, int part, float a, float b, float got, float want) {
    if (atomicAdd(&R->diff[part], 1ull) == 0ull) { R->first[part][0] = bits(a); R->first[part][1] = bits(b); R->first[part][2] = bits(got); R->first[part][3] = bits(want); }
}

// one thread per mantissa
__global__ __launch_bounds__(256) void chain_kernel(Result *R) {
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;  // < 2^23: the grid is exactly 2^23 threads
    unsigned long long n = 0;
    for (int e = -40; e <= 40; e += 8) {
        const float b = from_bits(((m & 1u) << 31) | ((uint32_t)(127 + e) << 23) | m);
        const uint32_t h = hash32(m * 11u + (uint32_t)(e + 40));
        const float a = from_bits((h & 0x80000000u) | ((127u - 40u + (h >> 8) % 80u) << 23) | (hash32(h) & 0x7fffffu));  // |a| in [2^-40, 2^40)
        const float want = a / b, want1 = 1.0f / b;
        const float q = div_inrange(a, b), q2 = div_by(a, recip_refine(b)), q1 = div_inrange(1.0f, b);
        if (bits(q) != bits(want)) report(R, 0, a, b, q, want);
        if (bits(q2) != bits(want)) report(R, 0, a, b, q2, want);
        if (bits(q1) != bits(want1)) report(R, 0, 1.0f, b, q1, want1);
        n += 3;
    }
    atomicAdd(&R->cases[0], n);
    if (m == 0x7fffffu) {
        const float b = from_bits((127u << 23) | m);
        R->rcp_allones = __builtin_amdgcn_rcpf(b); R->div_allones = 1.0f / b; R->chain_allones = div_inrange(1.0f, b);
    }
}

// one block per W, its threads stride over x
__global__ __launch_bounds__(256) void const_kernel(Result *R, const float *rcp) {
    const uint32_t W = blockIdx.x + 1u;
    const float fw = (float)W, y = rcp[W];
    unsigned long long n = 0;
    for (uint32_t x = threadIdx.x; x < W; x += 256u, n++) {
        const float a = 2.0f * ((float)x + 0.5f);
        const float want = a / fw, got = div_const(a, fw, y);
        if (bits(got) != bits(want)) report(R, 1, a, fw, got, want);
    }
    atomicAdd(&R->cases[1], n);
}

__global__ __launch_bounds__(256) void dt_kernel(Result *R) {
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    unsigned long long n = 0;
    for (int k = 0; k < 2; k++) {
        const float d = from_bits(((m & 1u) << 31) | ((uint32_t)(k ? 127 - 21 : 126) << 23) | m);
        const float inv = div_inrange(1.0f, d), inv_generic = 1.0f / d;
        for (uint32_t s = 3; s <= 11u; s++) {
            const float fn = (float)(1u << s);
            const float want = 1.0f / (fn * fabsf(d));
            const float got = fabsf(inv) * pow2_recip(fn), got2 = fabsf(inv_generic) * pow2_recip(fn);
            if (bits(got) != bits(want)) report(R, 2, d, fn, got, want);
            if (bits(got2) != bits(want)) report(R, 2, d, fn, got2, want);
            n += 2;
        }
    }
    atomicAdd(&R->cases[2], n);
}

int main() {
    const uint32_t Wmax = 8192;
    std::vector<float> rcp(Wmax + 1, 0.0f);
    for (uint32_t W = 1; W <= Wmax; W++) rcp[W] = 1.0f / (float)W;
    Result *d_R = nullptr, R;
    float *d_rcp = nullptr;
    CHECK(hipMalloc(&d_R, sizeof(Result)));
    CHECK(hipMemset(d_R, 0, sizeof(Result)));
    CHECK(hipMalloc(&d_rcp, rcp.size() * sizeof(float)));
    CHECK(hipMemcpy(d_rcp, rcp.data(), rcp.size() * sizeof(float), hipMemcpyHostToDevice));
    chain_kernel<<<(1u << 23) / 256u, 256>>>(d_R);
    const_kernel<<<Wmax, 256>>>(d_R, d_rcp);
    dt_kernel<<<(1u << 23) / 256u, 256>>>(d_R);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&R, d_R, sizeof(Result), hipMemcpyDeviceToHost));
    const char *names[3] = {"chain", "const", "dt"};
    for (int p = 0; p < 3; p++) {
        printf("%s: %llu cases, %llu differences\n", names[p], R.cases[p], R.diff[p]);
        if (R.diff[p]) printf("  first: operands %08x %08x got %08x want %08x\n", R.first[p][0], R.first[p][1], R.first[p][2], R.first[p][3]);
    }
    printf("1 / 0x1.fffffep0: v_rcp_f32 %a, the device's division %a, div_inrange %a\n", R.rcp_allones, R.div_allones, R.chain_allones);
    (void)hipFree(d_R); (void)hipFree(d_rcp);
    return 0;
}
