// lds_atomic64_probe.hip -- the rate of 64-bit LDS atomic adds (ds_add_u64) against the 32-bit ones
// (ds_add_u32) on the slotted digit histogram of kth.hip: h[digit * SLOTS + (tid & (SLOTS - 1))], 1024
// threads, 16 adds per thread and round, as a level of the one-launch select issues them
// (DESIGN.md §3.23).  Digits: uniform over 256, over 4 values (the top digit of probabilities), or
// one value.  Prints ns per round and workgroup and adds per ns and CU, one workgroup per CU.
//   hipcc --offload-arch=gfx950 -O3 -o harness/bin/lds_atomic64_probe harness/exp/lds_atomic64_probe.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                         \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));    \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

constexpr int BLOCK = 1024, KPT = 16;

template <typename W, int SLOTS>
__global__ __launch_bounds__(BLOCK) void k_probe(const uint32_t *digits, int rounds, unsigned long long *sink) {
    __shared__ W h[256 * SLOTS];
    const uint32_t tid = threadIdx.x;
    uint32_t d[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) d[j] = digits[(size_t)j * BLOCK + tid] & 255u;
    for (uint32_t i = tid; i < 256u * SLOTS; i += BLOCK) h[i] = 0;
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) atomicAdd(&h[d[j] * SLOTS + (tid & (SLOTS - 1u))], (W)(d[j] + 1u + (uint32_t)r));
        __syncthreads();
    }
    unsigned long long s = 0;
    for (uint32_t i = tid; i < 256u * SLOTS; i += BLOCK) s += (unsigned long long)h[i];
    if (s == 0x123456789ull) sink[blockIdx.x] = s;  // (keeps the adds alive)
}

template <typename W, int SLOTS>
void measure(const char *name, const uint32_t *d_digits, const char *dist, unsigned long long *sink, int cus) {
    const int rounds = 2000;
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    k_probe<W, SLOTS><<<cus, BLOCK>>>(d_digits, 10, sink);
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
        CHECK(hipEventRecord(a));
        k_probe<W, SLOTS><<<cus, BLOCK>>>(d_digits, rounds, sink);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (ms < best) best = ms;
    }
    const double ns_round = best * 1e6 / rounds;
    printf("%-8s slots %2d  %-8s %8.1f ns per round of %d adds  %6.2f adds/ns/CU\n", name, SLOTS, dist, ns_round, BLOCK * KPT,
           BLOCK * KPT / ns_round);
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("# %s, %d CUs, one workgroup of %d threads per CU, best of 5\n", prop.name, cus, BLOCK);
    const size_t n = (size_t)BLOCK * KPT;
    uint32_t *host = (uint32_t *)malloc(n * 4), *d_digits;
    unsigned long long *sink;
    CHECK(hipMalloc(&d_digits, n * 4));
    CHECK(hipMalloc(&sink, (size_t)cus * 8));
    const char *dists[3] = {"uniform", "four", "one"};
    for (int di = 0; di < 3; ++di) {
        uint64_t s = 0x9E3779B97F4A7C15ull;
        for (size_t i = 0; i < n; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t r = (uint32_t)(s >> 33);
            host[i] = di == 0 ? r & 255u : di == 1 ? 120u + (r & 3u) : 77u;
        }
        CHECK(hipMemcpy(d_digits, host, n * 4, hipMemcpyHostToDevice));
        measure<uint32_t, 32>("u32", d_digits, dists[di], sink, cus);
        measure<uint32_t, 16>("u32", d_digits, dists[di], sink, cus);
        measure<unsigned long long, 16>("u64", d_digits, dists[di], sink, cus);
        measure<unsigned long long, 8>("u64", d_digits, dists[di], sink, cus);
    }
    CHECK(hipFree(d_digits));
    CHECK(hipFree(sink));
    free(host);
    return 0;
}
