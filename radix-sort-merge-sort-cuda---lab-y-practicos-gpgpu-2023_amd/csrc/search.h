// search.h -- ranks of values in sorted rows (search.hip: labsort_searchsorted_device): shapes, the
// sample table of the long path, the order image of a 2-byte key word.
#pragma once
#include "../../include/labsort.h"
#include "common.h"
#include "unique.h"

namespace labsort {

// ---- shapes: a workgroup of SS_BLOCK threads walks chunks of SS_CHUNK consecutive values of one
// row; thread t of a chunk owns values t * SS_VPT .. + SS_VPT - 1 and runs their searches side by
// side.  Two such workgroups (16 waves) fit a CU beside SS_LDS_BYTES of images each.
constexpr int SS_BLOCK = 512;
constexpr int SS_VPT = 8;  // values per thread: 16, 32 or 64 bytes of 2-, 4- or 8-byte keys
constexpr int SS_CHUNK = SS_BLOCK * SS_VPT;  // 4096
constexpr int SS_LDS_BYTES = 64 * 1024;      // images of the longest sequence the LDS path takes
constexpr int SS_LDS_WG_PER_CU = 2;          // grid cap of the LDS path with a shared sequence
constexpr int SS_LONG_WG_PER_CU = 4;         // and of the long path (8 to 32 KB of samples each)

// ---- the long path's sample table: sample j of a sequence of cols elements is the image of the
// last element of stride j, strides of ss_stride(cols) elements; ss_strides(cols) of them hold an
// element (the last one may be partial), the table's slots behind them repeat the last element.
constexpr int SS_SAMPLES = 4096;
constexpr int SS_SAMPLE_BLOCK = 256;
__host__ __device__ inline uint32_t ss_stride(uint32_t cols) { return (cols + SS_SAMPLES - 1) / SS_SAMPLES; }
__host__ __device__ inline uint32_t ss_strides(uint32_t cols) { return (cols + ss_stride(cols) - 1) / ss_stride(cols); }
static_assert(SS_SAMPLES % SS_SAMPLE_BLOCK == 0 && SS_SAMPLES * 8 <= SS_LDS_BYTES, "the table fits the LDS array");

// ---- counting (labsort_bucket_counts_device, labsort_bincount_device): the ranks go into counters.
// The LDS path keeps the edges' images and nedges + 1 32-bit counters side by side in BC_LDS_BYTES,
// so that two workgroups fit a CU's 160 KB: bc_row_edges(sizeof(key)) edges at the most, a multiple
// of 64 (10176 4-byte, 6784 8-byte, 13632 2-byte), never below SS_SAMPLES.  Bincount has counters
// only: BIN_ROW_BINS + 1 of them.
constexpr int BC_LDS_BYTES = 80 * 1024;
__host__ __device__ constexpr uint32_t bc_row_edges(size_t esz) { return (uint32_t)((BC_LDS_BYTES - 4) / (esz + 4) / 64 * 64); }
constexpr int BIN_ROW_BINS = 16384;
static_assert(bc_row_edges(8) >= SS_SAMPLES && bc_row_edges(2) * 6 + 4 <= BC_LDS_BYTES, "the counting LDS path's limits");
// LABSORT_BC_COMBINE=0 (an A/B build): one atomic per value instead of one per run of equal
// neighbouring ranks of a thread
#ifndef LABSORT_BC_COMBINE
#define LABSORT_BC_COMBINE 1
#endif

// ---- the order image of a key word K: UqImage<K> (unique.h) for 4- and 8-byte words; for the 2-byte
// words of BF16 / F16 ord16 (common.h), what labsort_key_order_bits computes for them.
struct SsImage16 {
    uint32_t nan_t;
    __host__ __device__ uint16_t ord(uint16_t x) const { return (uint16_t)ord16(x, nan_t); }
};

}  // namespace labsort
