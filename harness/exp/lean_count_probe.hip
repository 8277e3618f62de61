// lean_count_probe.hip -- where k_hist_lean's time goes: its counting loop on
// 2^28 uniform uint32 keys, 256 workgroups of 1024 threads, each reading one contiguous 4 MiB
// part, with pieces of the work switched off.  Standalone (no labsort code); timing only.
// Results: profiles/count_pipeline_probe.txt.
//   LOOP 0: the library's loop (next group loaded under an `if`, c = x after the count: vmcnt(0) before the count)
//        1: prologue / two-group steady loop / peeled end, registers swap roles (vmcnt(NU); measured, not kept)
//        2: no prefetch: load a group, count it
//   NU:   uint4 per thread and group (2, 4 or 8)
//   H2:   digit-2 counters, 32 replicas (one LDS atomic per key)
//   HT:   top-14-bit counters, plain (one LDS atomic per key)
//   FL:   flush: 16384 + 256 device atomics per workgroup
//   FENCE: the kernel's end -- a ticket behind the flush, the last workgroup sums the counts it sees
//        0: none
//        1: __threadfence() in every thread, barrier, ticket (k_hist_lean before this probe)
//        2: s_waitcnt vmcnt(0) in every thread, barrier, ticket, no fence
//        3: s_waitcnt vmcnt(0) in every thread, barrier, thread 0 fences and draws the ticket (k_hist_lean now)
//        4: barrier, thread 0 fences and draws the ticket: no wave but thread 0's waits for its atomics.  NOT a
//           correct end; here only to time what the per-wave wait of 3 costs.  Its sum check proves nothing.
//   Every FENCE run counts the launches whose last workgroup saw a sum other than n (a sanity check of the
//   probe: a rare ordering miss would not show in a hundred launches).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o lean_count_probe lean_count_probe.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

constexpr int HB = 1024, SL = 32, TOP = 16384;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 ldnt(const uint4 *p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

__global__ void k_fill(uint32_t *k, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        k[i] = (uint32_t)(z >> 32);
    }
}

template <int LOOP, int NU, bool H2, bool HT, bool FL, int FENCE>
__global__ __launch_bounds__(HB) void k_count(const uint32_t *__restrict__ keys, size_t n, uint32_t *__restrict__ out) {
    __shared__ uint32_t h2[256 * SL];
    __shared__ uint32_t ht[TOP];
    const uint32_t t = threadIdx.x;
    for (int i = t; i < 256 * SL; i += HB) h2[i] = 0u;
    for (int i = t; i < TOP; i += HB) ht[i] = 0u;
    __syncthreads();
    const uint32_t slot = t & (SL - 1);
    uint32_t ka = ~0u, ko = 0u;
    auto countg = [&](const uint4 (&c)[NU]) {
        uint32_t k[4 * NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            k[4 * u] = c[u].x; k[4 * u + 1] = c[u].y; k[4 * u + 2] = c[u].z; k[4 * u + 3] = c[u].w;
        }
#pragma unroll
        for (int j = 0; j < 4 * NU; ++j) { ka &= k[j]; ko |= k[j]; }
        if (H2) {
#pragma unroll
            for (int j = 0; j < 4 * NU; ++j) atomicAdd(&h2[((k[j] >> 16) & 255u) * SL + slot], 1u);
        }
        if (HT) {
#pragma unroll
            for (int j = 0; j < 4 * NU; ++j) atomicAdd(&ht[k[j] >> 18], 1u);
        }
    };
    const size_t per = n / gridDim.x, nv = per / 4;
    const uint4 *v = reinterpret_cast<const uint4 *>(keys + blockIdx.x * per);
    size_t i = t;
    uint4 c[NU], x[NU];
    auto load = [&](uint4 (&g)[NU], size_t at) {
#pragma unroll
        for (int u = 0; u < NU; ++u) g[u] = ldnt(v + at + u * HB);
        if (LOOP == 1) __builtin_amdgcn_sched_barrier(0);
    };
    if (LOOP == 0) {
        if (i + (NU - 1) * HB < nv) load(c, i);
        for (; i + (NU - 1) * HB < nv; i += NU * HB) {
            if (i + (2 * NU - 1) * HB < nv) load(x, i + NU * HB);
            countg(c);
#pragma unroll
            for (int u = 0; u < NU; ++u) c[u] = x[u];
        }
    } else if (LOOP == 1) {
        if (i + (NU - 1) * HB < nv) {
            load(c, i);
            for (; i + (3 * NU - 1) * HB < nv; i += 2 * NU * HB) {
                load(x, i + NU * HB);
                countg(c);
                load(c, i + 2 * NU * HB);
                countg(x);
            }
            if (i + (2 * NU - 1) * HB < nv) {
                load(x, i + NU * HB);
                countg(c);
                countg(x);
            } else {
                countg(c);
            }
        }
    } else {
        for (; i + (NU - 1) * HB < nv; i += NU * HB) {
            load(c, i);
            countg(c);
        }
    }
    __syncthreads();
    if (t < 256u) {
        uint32_t s = 0;
#pragma unroll 8
        for (int q = 0; q < SL; ++q) s += h2[t * SL + ((q + t) & (SL - 1))];
        if (s) atomicAdd(&out[TOP + t], s);
    }
    if (FL) {
        const uint32_t rot = (blockIdx.x * 1088u) & (uint32_t)(TOP - 1);
        for (uint32_t i0 = t; i0 < (uint32_t)TOP; i0 += HB) {
            const uint32_t j = (i0 + rot) & (uint32_t)(TOP - 1);
            const uint32_t s = ht[j];
            if (s) atomicAdd(&out[j], s);
        }
    }
    if ((ka & ~ko) == 0x12345u) out[0] = ka;  // keeps the AND / OR alive
    if (FENCE) {
        __shared__ uint32_t last;
        if (FENCE == 1) __threadfence();
        if (FENCE == 2 || FENCE == 3) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's atomics have been performed
        __syncthreads();
        if (t == 0) {
            if (FENCE >= 3) __threadfence();
            last = atomicAdd(&out[TOP + 256], 1u) == gridDim.x - 1u;
        }
        __syncthreads();
        if (!last) return;
        __threadfence();
        uint32_t s = 0;
        for (uint32_t j = t; j < (uint32_t)TOP; j += HB) s += __hip_atomic_load(&out[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(&out[TOP + 257], s);
    }
}

template <class F, class G>
float timeit(int reps, F f, G after) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    std::vector<float> ts;
    for (int r = 0; r < reps + 2; ++r) {
        (void)hipEventRecord(a);
        f();
        (void)hipEventRecord(b);
        (void)hipEventSynchronize(b);
        float ms;
        (void)hipEventElapsedTime(&ms, a, b);
        if (r >= 2) ts.push_back(ms);
        after();
    }
    std::sort(ts.begin(), ts.end());
    printf("median %.4f min %.4f max %.4f ms", ts[ts.size() / 2], ts.front(), ts.back());
    return ts[ts.size() / 2];
}

int main() {
    const size_t n = (size_t)1 << 28;
    uint32_t *keys, *out;
    CK(hipMalloc(&keys, n * 4));
    CK(hipMalloc(&out, (TOP + 258) * 4));
    CK(hipMemset(out, 0, (TOP + 258) * 4));
    k_fill<<<4096, 256>>>(keys, n);
    CK(hipDeviceSynchronize());
#define RUN(L, NU, H2, HT, FL) \
    printf("loop %d nu %d h2 %d ht %d flush %d  ", L, NU, H2, HT, FL); \
    { const float t_ = timeit(11, [&] { k_count<L, NU, H2, HT, FL, 0><<<256, HB>>>(keys, n, out); }, [] {}); \
      printf("  %6.0f GB/s\n", 4.0 * n / 1e6 / t_); } \
    CK(hipDeviceSynchronize());
    RUN(0, 4, false, false, false) RUN(1, 4, false, false, false) RUN(2, 4, false, false, false)
    RUN(0, 4, true, false, false) RUN(0, 4, false, true, false) RUN(0, 4, false, true, true)
    RUN(0, 4, true, true, false)
    RUN(0, 4, true, true, true) RUN(1, 4, true, true, true) RUN(2, 4, true, true, true)
    RUN(0, 2, true, true, true) RUN(1, 2, true, true, true)
    RUN(0, 8, true, true, true) RUN(1, 8, true, true, true)
    // the kernel's end: the counters zeroed before every launch, the last workgroup's sum read after it
#define RUNF(F) \
    printf("fence %d  ", F); \
    { uint32_t bad = 0, seen = 0; \
      CK(hipMemset(out, 0, (TOP + 258) * 4)); \
      const float t_ = timeit(101, [&] { k_count<0, 4, true, true, true, F><<<256, HB>>>(keys, n, out); }, \
                              [&] { uint32_t r_[2]; (void)hipMemcpy(r_, out + TOP + 256, 8, hipMemcpyDeviceToHost); \
                                    seen += r_[0] == 256u; bad += F != 0 && (r_[0] != 256u || r_[1] != (uint32_t)n); \
                                    (void)hipMemset(out, 0, (TOP + 258) * 4); }); \
      printf("  %6.0f GB/s  launches checked %u, wrong sums seen by the last workgroup: %u\n", 4.0 * n / 1e6 / t_, seen, bad); } \
    CK(hipDeviceSynchronize());
    RUNF(0) RUNF(1) RUNF(2) RUNF(3) RUNF(4) RUNF(1) RUNF(3)
    return 0;
}
