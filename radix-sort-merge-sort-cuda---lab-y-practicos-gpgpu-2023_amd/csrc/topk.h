// topk.h -- top-k selection (topk.hip): shapes.
#pragma once
#include "common.h"

namespace labsort {

// ---- radix select, MSD first, 8-bit digits (rows longer than the segmented sort's pair tile) ----
constexpr int TK_BLOCK = 1024;
constexpr int TK_CHUNK = 16384;   // keys per (chunk, row) workgroup: the other passes' tile
constexpr int TK_LEVELS = 4;
constexpr int TK_SLOTS = 32;      // LDS counter replicas per digit: one per bank, as k_histogram
// A row's level histogram is added to by at most this many workgroups (each then counts several
// consecutive chunks and adds once): 2^28 keys in one row would otherwise put 16384 x 256 atomic
// adds on 256 words, that is on eight L2 lines.
constexpr uint32_t TK_MAX_HIST_WG = 1024;
// Narrowing: a row whose chosen bucket holds at most cols / TK_CAND_DIV keys is copied to the
// row's candidate buffer of that capacity ((u, position) pairs: 8 bytes each, so the buffer costs
// cols bytes per row) and every later level reads the buffer.  Random keys narrow after level 0
// to cols / 256 keys; 1/8 still leaves each later level with an eighth of the row to read.
constexpr int TK_CAND_DIV = 8;
// Large k: from k > cols / TK_SORT_DIV the call sorts whole rows and copies the first k
// (LABSORT_TOPK_SORT_DIV in labsort.h; DESIGN.md §3.7 has the sweep).
constexpr int TK_SORT_DIV = 4;
constexpr int TK_HDR_BYTES = 256;  // word 0: an inner sort reported an error; the short path's class
                                   // counts sit where the segmented sort keeps them (SEG_HDR_CNT)

}  // namespace labsort
