// Micro-benchmark: a plain streaming read -- the sum of an array with 16-byte loads, four in flight per lane, 8 workgroups of 256 per CU in a
// grid-stride loop -- as the yardstick tools/hist_quick.py sets vk_volume_histogram against.  Calibration only -- not part of the product.
//
//   hipcc --offload-arch=gfx950 -O3 -o stream_read tools/ubench/stream_read.hip && ./stream_read BYTES [BYTES ...]
// prints one JSON object {"<bytes>": <best ms of 3 groups of 10 reads>, ...}.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1);} } while (0)

__global__ __launch_bounds__(256) void stream_read_kernel(const uint4 *__restrict__ p, size_t n, unsigned *out) {
    const size_t stride = (size_t)gridDim.x * 256u;
    unsigned acc = 0u;
    size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    for (; i + 3u * stride < n; i += 4u * stride) {
        const uint4 a = p[i], b = p[i + stride], c = p[i + 2u * stride], d = p[i + 3u * stride];
        acc += (a.x + a.y + a.z + a.w) + (b.x + b.y + b.z + b.w) + (c.x + c.y + c.z + c.w) + (d.x + d.y + d.z + d.w);
    }
    for (; i < n; i += stride) { const uint4 a = p[i]; acc += a.x + a.y + a.z + a.w; }
    if (acc == 0x9e3779b9u) *out = acc;  // (keeps the loads; the array holds ones)
}

int main(int argc, char **argv) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const unsigned grid = (unsigned)prop.multiProcessorCount * 8u;
    unsigned *out;
    CHECK(hipMalloc(&out, 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("{");
    for (int k = 1; k < argc; k++) {
        const size_t bytes = strtoull(argv[k], nullptr, 0) & ~(size_t)15, n = bytes / 16;
        void *p;
        CHECK(hipMalloc(&p, bytes ? bytes : 16));
        CHECK(hipMemset(p, 1, bytes));
        for (int w = 0; w < 3; w++) hipLaunchKernelGGL(stream_read_kernel, dim3(grid), dim3(256), 0, 0, (const uint4 *)p, n, out);
        CHECK(hipDeviceSynchronize());
        float best = 1e9f;
        for (int g = 0; g < 3; g++) {
            CHECK(hipEventRecord(e0, 0));
            for (int it = 0; it < 10; it++) hipLaunchKernelGGL(stream_read_kernel, dim3(grid), dim3(256), 0, 0, (const uint4 *)p, n, out);
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            best = ms / 10.0f < best ? ms / 10.0f : best;
        }
        CHECK(hipFree(p));
        printf("%s\"%zu\": %.4f", k > 1 ? ", " : "", bytes, best);
    }
    printf("}\n");
    return 0;
}
