// sort16.h -- the two-pass radix sort of long 16-bit rows (sort16.hip): shapes, and what it shares
// with the row sort (rowsort.hip).
#pragma once
#include "common.h"

namespace labsort {

// ---- long rows: two stable LSD passes with 8-bit digits on u = ord16(key) ^ x16 ----
// One workgroup per (row, chunk) in the count and the scatter kernels; a chunk is up to S16_CHUNK
// consecutive keys of one row, 16 per thread.
#ifndef LABSORT_S16_BLOCK
#define LABSORT_S16_BLOCK 1024  // threads per (row, chunk) workgroup (A/B build knob: 512 = 8192-key chunks)
#endif
#ifndef LABSORT_S16_KPT
#define LABSORT_S16_KPT 16  // keys per thread (A/B build knob: 8 = 8192-key chunks of 1024 threads, two per CU)
#endif
constexpr int S16_BLOCK = LABSORT_S16_BLOCK;
constexpr int S16_KPT = LABSORT_S16_KPT;
constexpr int S16_CHUNK = S16_BLOCK * S16_KPT;  // 16384 keys
// (the count table, its scan and their constants, what the shapes must satisfy: chunk_pass.h)

// rowsort.hip: the LDS path of labsort_sort_rows_device behind its argument checks, for a shape
// that rs_lds_path takes; d_ws: the 256-byte header.  labsort_sort16_device forwards its short
// rows here.
int sort_rows_lds(const void *d_keys, size_t rows, size_t cols, int descending, int key_type, void *d_keys_out,
                  uint32_t *d_idx_out, void *d_ws, hipStream_t s);

}  // namespace labsort
