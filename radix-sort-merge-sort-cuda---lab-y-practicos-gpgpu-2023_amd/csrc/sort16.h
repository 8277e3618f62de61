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
#ifndef LABSORT_S16_PAIR
#define LABSORT_S16_PAIR 0  // 1: aligned neighbours of a run leave the scatter as one 4-byte store (A/B build knob)
#endif
constexpr int S16_PAIR = LABSORT_S16_PAIR;
constexpr int S16_BLOCK = LABSORT_S16_BLOCK;
constexpr int S16_KPT = LABSORT_S16_KPT;
constexpr int S16_CHUNK = S16_BLOCK * S16_KPT;  // 16384 keys
static_assert(S16_KPT % 2 == 0 && S16_BLOCK % 256 == 0, "ranks are packed in pairs; 256 threads hold the digits");
static_assert(S16_CHUNK <= 65536, "a key's place in its chunk travels through LDS as 16 bits");
constexpr int S16_SLOTS = 32;  // LDS counter replicas per digit in the count kernel: one per bank, as k_tk_hist
// The scan along the chunk axis of the count table [row][digit][chunk]: up to S16_SCAN_SERIAL
// chunks per row one thread per (row, digit) walks its run of the table; above, one workgroup per
// (row, digit) scans it in steps of S16_SCAN_BLOCK chunks.
constexpr uint32_t S16_SCAN_SERIAL = 64;
constexpr int S16_SCAN_BLOCK = 1024;

// rowsort.hip: the LDS path of labsort_sort_rows_device behind its argument checks, for a shape
// that rs_lds_path takes; d_ws: the 256-byte header.  labsort_sort16_device forwards its short
// rows here.
int sort_rows_lds(const void *d_keys, size_t rows, size_t cols, int descending, int key_type, void *d_keys_out,
                  uint32_t *d_idx_out, void *d_ws, hipStream_t s);

}  // namespace labsort
