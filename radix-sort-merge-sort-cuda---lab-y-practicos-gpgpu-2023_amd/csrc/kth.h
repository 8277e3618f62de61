// kth.h -- k-th key selection per row (kth.hip): shapes.
#pragma once
#include "common.h"
#include "topk.h"

namespace labsort {

constexpr int KTH_BLOCK = TK_BLOCK;     // every kernel of kth.hip: 1024 threads
constexpr int KTH_KPT = 16;             // keys a thread of the one-launch kernel holds in registers
constexpr int KTH_ROW_KEYS = TK_CHUNK;  // longest row of the one-launch path (labsort_kth_row_keys)
static_assert(KTH_ROW_KEYS == KTH_BLOCK * KTH_KPT, "a short row is held in the registers of one workgroup");
// Rows of up to KTH_SMALL_BLOCK * KTH_KPT keys: the one-launch kernel with a smaller workgroup and
// fewer counter replicas, so that a thread still holds 16 keys and a level clears and folds 2048
// LDS words, not 8192 (DESIGN.md §3.16 has the A/B; LABSORT_KTH_SMALL=0 builds without it).
#ifndef LABSORT_KTH_SMALL
#define LABSORT_KTH_SMALL 1
#endif
constexpr int KTH_SMALL_BLOCK = 256;
constexpr int KTH_SMALL_SLOTS = 8;
constexpr int KTH_SMALL_ROW_KEYS = LABSORT_KTH_SMALL ? KTH_SMALL_BLOCK * KTH_KPT : 0;
constexpr int KTH_HDR_BYTES = TK_HDR_BYTES;  // word 0: a d_k[r] outside [1, cols] was clamped
// The one-launch top-k filter skips its ordered scan of the threshold's ties when all of them are
// kept (DESIGN.md §3.22 has the A/B; LABSORT_TKM_SKIP_SCAN=0 builds with the scan always run).
#ifndef LABSORT_TKM_SKIP_SCAN
#define LABSORT_TKM_SKIP_SCAN 1
#endif
// Top-p filtering (labsort_top_p_device): the select's histograms hold masses, 64-bit words of
// 2^-40 fixed point, so a slot costs twice the LDS of a counter: half the replicas of the count
// kernels at 1024 threads (32 KB, the size of their histogram), the same eight at 256 (16 KB;
// 16 were 17-30 % slower on rows of 1024 and 4096 keys).
constexpr int TP_FRAC_BITS = 40;       // a weight is floor(x 2^40), at most 2^40
constexpr size_t TP_MAX_COLS = 1u << 23;  // so that a row's total stays below 2^63
constexpr int TP_SLOTS = TK_SLOTS / 2;
#ifndef LABSORT_TP_SMALL_SLOTS
#define LABSORT_TP_SMALL_SLOTS 8  // (A/B build knob)
#endif
constexpr int TP_SMALL_SLOTS = LABSORT_TP_SMALL_SLOTS;
// Categorical sampling (labsort_sample_device): the weights and the column limit of top-p filtering,
// so a long row has at most 512 chunks, which one workgroup of as many threads scans (k_smp_pick).
constexpr int SMP_MAX_CHUNKS = (int)(TP_MAX_COLS / TK_CHUNK);
// One workgroup per row (short rows) or per draw (long rows): up to 2^31 - 1 of them, launched
// SMP_MAX_GRID at a time, 2^31 threads at 1024 a workgroup.
constexpr unsigned SMP_MAX_GRID = 1u << 21;
static_assert((unsigned long long)SMP_MAX_GRID * KTH_BLOCK < (1ull << 32), "the runtime's limit on a grid's threads");
static_assert(SMP_MAX_CHUNKS == 512 && SMP_MAX_CHUNKS <= KTH_BLOCK, "one thread per chunk of the longest row");

}  // namespace labsort
