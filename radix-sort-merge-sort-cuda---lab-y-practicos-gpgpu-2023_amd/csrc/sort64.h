// sort64.h -- the sort of 8-byte keys (sort64.hip): the order images, shapes, the device-side plan.
#pragma once
#include "../../include/labsort.h"
#include "common.h"

namespace labsort {

// ---- float64 keys (LABSORT_KEY_F64): the order image of an IEEE-754 binary64 word, f32_ord
// (common.h) at 64 bits.  Plain uint64 order on f64_ord(x) is -inf < ... < -0.0 < +0.0 < ... <
// +inf < NaN, every NaN equal (~0); f64_unord inverts it for every non-NaN word and gives the NaN
// image back as 0x7FFFFFFFFFFFFFFF.  The one definition: the kernels and labsort_key_order_bits64
// compile this.
constexpr uint64_t S64_SIGN = 0x8000000000000000ull;
__host__ __device__ inline uint64_t f64_ord(uint64_t x) {
    if ((x & ~S64_SIGN) > 0x7FF0000000000000ull) return ~0ull;
    return (x & S64_SIGN) ? ~x : x | S64_SIGN;
}
__host__ __device__ inline uint64_t f64_unord(uint64_t o) { return (o >> 63) ? o & ~S64_SIGN : ~o; }
// The image of a key word of one of the three 8-byte key types, and its inverse (kt: LABSORT_KEY_*;
// another value gives the word back)
__host__ __device__ inline uint64_t key64_ord(uint64_t x, int kt) {
    return kt == LABSORT_KEY_F64 ? f64_ord(x) : kt == LABSORT_KEY_I64 ? x ^ S64_SIGN : x;
}
__host__ __device__ inline uint64_t key64_unord(uint64_t o, int kt) {
    return kt == LABSORT_KEY_F64 ? f64_unord(o) : kt == LABSORT_KEY_I64 ? o ^ S64_SIGN : o;
}

// ---- shapes: one workgroup per row (cols <= S64_CHUNK) or per (row, chunk) of up to S64_CHUNK
// consecutive keys, 8 per thread: 64 KB of keys, 32 KB of positions and 16 KB of per-wave
// counters in LDS.
#ifndef LABSORT_S64_BLOCK
#define LABSORT_S64_BLOCK 1024  // threads per workgroup (A/B build knob)
#endif
#ifndef LABSORT_S64_KPT
#define LABSORT_S64_KPT 8  // keys per thread (A/B build knob)
#endif
constexpr int S64_BLOCK = LABSORT_S64_BLOCK;
constexpr int S64_KPT = LABSORT_S64_KPT;
constexpr int S64_CHUNK = S64_BLOCK * S64_KPT;  // 8192 keys
// (the count table, its scan and their constants, what the shapes must satisfy: chunk_pass.h)

// ---- the plan of a long-path call, decided on the device (k_s64_plan) from the OR of u and the
// OR of ~u over every key of the call: byte p varies where (or_u & or_n) has a bit of byte p.
constexpr uint32_t S64_IN = 0, S64_OUT = 1, S64_TMP = 2;  // a pass's source and destination
struct S64Plan {
    unsigned long long or_u, or_n;  // zeroed by the call, ORed into by k_s64_bits
    uint32_t mask;                  // bit p: the pass on byte p of the image runs
    uint32_t m;                     // the number of those
    uint32_t src[8], dst[8];        // of pass p, where it is active: S64_*
    uint32_t last[8];               // 1: pass p is the last active one (it stores keys, not images)
};
constexpr size_t S64_PLAN_BYTES = 256;
static_assert(sizeof(S64Plan) <= S64_PLAN_BYTES, "the plan's region");
// word of the 256-byte header that k_s64_plan copies the mask to (labsort_sort64_passes; the
// short path leaves it cleared).  Word 0 is the status word of every dense entry.
constexpr uint32_t S64_HDR_MASK = 2;

}  // namespace labsort
