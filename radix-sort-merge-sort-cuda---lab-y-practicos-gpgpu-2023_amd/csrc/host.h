// host.h -- what every host driver of liblabsort.so needs, each defined once (internal: every
// .hip file with an entry of the C ABI or a launch, and the headers that launch: seg_kernels.h,
// chunk_pass.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/labsort.h"
#include "common.h"

namespace labsort {

// records e for labsort_last_hip_error (api.hip's thread-local slot); returns LABSORT_ERR_HIP
int fail_hip(hipError_t e);
#define HIP_TRY(x)                                            \
    do {                                                      \
        hipError_t _e = (x);                                  \
        if (_e != hipSuccess) return ::labsort::fail_hip(_e); \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline uint32_t flip_of(int key_type) { return key_type == LABSORT_KEY_I32 ? 0x80000000u : 0u; }
inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline bool key_type_ok(int key_type) { return key_type == LABSORT_KEY_U32 || key_type == LABSORT_KEY_I32; }
// The entries that also order float32 keys: the device sorts, the segmented sorts and top-k.  F32
// has no uniform flip (flip_of gives 0): those entries apply f32_ord / f32_unord (common.h)
// where a key enters and leaves, and everything between orders the image as uint32.
inline bool device_key_type_ok(int key_type) { return key_type_ok(key_type) || key_type == LABSORT_KEY_F32; }
// Top-k alone also takes 16-bit float keys (2-byte elements): it widens them to
// ord16(key) << 16 where it reads the input, so everything behind that orders uint32 as before.
inline bool key_type_is16(int key_type) { return key_type == LABSORT_KEY_BF16 || key_type == LABSORT_KEY_F16; }
inline uint32_t nan_t16(int key_type) { return key_type == LABSORT_KEY_BF16 ? BF16_NAN_T : F16_NAN_T; }
inline bool topk_key_type_ok(int key_type) { return device_key_type_ok(key_type) || key_type_is16(key_type); }
inline bool key_type_is64(int kt) { return kt == LABSORT_KEY_U64 || kt == LABSORT_KEY_I64 || kt == LABSORT_KEY_F64; }  // (sort64.hip alone)
// Key/value calls are in place only as a whole: one side aliased and the other not would
// read payloads that the key side's passes already overwrote.  Keys and payloads never
// share their output.
inline bool pairs_alias_ok(const void *ki, const void *vi, const void *ko, const void *vo) {
    return (ki == ko) == (vi == vo) && ko != vo;
}

// Compute units of the current device, asked once per process (256 where the runtime will not say; hidden: one copy)
__attribute__((visibility("hidden"))) inline int cu_count() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
    }
    return cus;
}

// Do the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte?
inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}

// The argument checks of a dense call (top-k, row sort, the 16- and 64-bit sorts) that reads rows x
// cols keys and writes rows x k keys and, with idx_out, as many 32-bit positions; rows, k != 0, and
// key_type is one that the entry takes: it gives the element's size, to which 2- and 8-byte keys
// must be aligned.  LABSORT_OK or LABSORT_ERR_ARG.
inline int dense_rows_args(const void *keys, size_t rows, size_t cols, size_t k, int key_type, const void *keys_out,
                           const void *idx_out) {
    if (!keys || !keys_out) return LABSORT_ERR_ARG;
    const size_t esz = key_type_is16(key_type) ? 2 : key_type_is64(key_type) ? 8 : 4;  // bytes per key
    if (esz != 4 && (((uintptr_t)keys | (uintptr_t)keys_out) & (esz - 1))) return LABSORT_ERR_ARG;
    if (k > cols || rows > (size_t)0x7FFFFFFFu / cols) return LABSORT_ERR_ARG;
    if (idx_out == keys_out) return LABSORT_ERR_ARG;
    if (ranges_overlap(keys, rows * cols * esz, keys_out, rows * k * esz)) return LABSORT_ERR_ARG;
    if (idx_out && ranges_overlap(keys, rows * cols * esz, idx_out, rows * k * 4)) return LABSORT_ERR_ARG;
    return LABSORT_OK;
}

// Timing scope: with labsort_timing_enable(1), an event pair on s around the launches made
// while the scope lives, counted under kernel class cls (api.hip keeps the state).
constexpr int LABSORT_K_UNTIMED = -1;  // a scope that records nothing
struct TimingScope {
    int cls;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    TimingScope(int c, hipStream_t st);
    ~TimingScope();
};

// Workspace carver: regions one behind the other, each starting on a 256-byte boundary.
struct Carver {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    }
};

// Status read of a workspace: waits for the stream, copies the workspace's first `count`
// words to `words`, waits again.  What the words mean is the caller's.
inline int read_ws_words(const void *d_ws, uint32_t *words, int count, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    if (!d_ws) return LABSORT_ERR_ARG;
    HIP_TRY(hipMemcpyAsync(words, d_ws, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return LABSORT_OK;
}

}  // namespace labsort
