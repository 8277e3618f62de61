// unique.h -- distinct keys with counts, first positions and inverse (unique.hip): shapes, the
// header word, the order image of a key word of either width.
#pragma once
#include "../../include/labsort.h"
#include "common.h"
#include "sort64.h"

namespace labsort {

// ---- shapes: one workgroup per chunk of UQ_CHUNK consecutive elements of the sorted array (of the
// input in consecutive mode).  Wave w owns elements w * UQ_WAVE_KEYS .. + UQ_WAVE_KEYS - 1 of the
// chunk and reads them in groups of 64 16-byte loads: lane l of group g holds the E = 16 /
// sizeof(key) consecutive elements from g * 64 E + l E on, so (wave, group, lane, k) in
// lexicographic order is the order of the elements.
constexpr int UQ_BLOCK = 1024;
constexpr int UQ_KPT = 8;  // keys per thread: two 16-byte loads of 4-byte keys, four of 8-byte keys
constexpr int UQ_W = UQ_BLOCK / WAVE;
constexpr int UQ_WAVE_KEYS = WAVE * UQ_KPT;
constexpr int UQ_CHUNK = UQ_BLOCK * UQ_KPT;  // 8192: a head's place in its chunk is 16 bits
static_assert(UQ_CHUNK <= 65536, "chunk-local places are stored as uint16_t");
constexpr int UQ_COUNTS_PER_WG = 4 * UQ_BLOCK;  // run lengths per workgroup of k_uq_counts

// ---- the workspace's 256-byte header.  Word 0 is the status word of every dense entry and stays
// clear; word UQ_HDR_SORT says which inner sort the last call ran on the region behind the header,
// written by the call's count kernel (labsort_unique_workspace_status asks that sort).
constexpr uint32_t UQ_HDR_SORT = 1;
constexpr uint32_t UQ_SORT_NONE = 0, UQ_SORT_KEYS = 1, UQ_SORT_PAIRS = 2, UQ_SORT_64 = 3;

// ---- the order image of a key word K = uint32_t (U32 / I32 / F32) or uint64_t (U64 / I64 / F64)
// and its inverse: what labsort_key_order_bits and labsort_key_order_bits64 compute.  Two keys are
// one value when their images are equal.
template <class K>
struct UqImage;
template <>
struct UqImage<uint32_t> {
    int kt;
    __host__ __device__ uint32_t ord(uint32_t x) const {
        return kt == LABSORT_KEY_F32 ? f32_ord(x) : kt == LABSORT_KEY_I32 ? x ^ 0x80000000u : x;
    }
    __host__ __device__ uint32_t unord(uint32_t o) const {
        return kt == LABSORT_KEY_F32 ? f32_unord(o) : kt == LABSORT_KEY_I32 ? o ^ 0x80000000u : o;
    }
};
template <>
struct UqImage<uint64_t> {
    int kt;
    __host__ __device__ uint64_t ord(uint64_t x) const { return key64_ord(x, kt); }
    __host__ __device__ uint64_t unord(uint64_t o) const { return key64_unord(o, kt); }
};

}  // namespace labsort
