// topk.h -- top-k selection (topk.hip): shapes, per-row state, workspace pointers and host launchers.
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

// Per row and level: what the level's kernels read.  Level L's scan writes entry L + 1, so no
// kernel reads a word that another workgroup of the same launch writes.
struct TkState {
    uint32_t prefix;    // digits chosen so far, in place (the top 8 * level bits)
    uint32_t krem;      // keys still to take among those that match the prefix (>= 1)
    uint32_t narrowed;  // 1: the source is the candidate buffer
    uint32_t ccount;    // pairs in the candidate buffer
    uint32_t sbase;     // survivors written so far (by the narrowing pass)
    uint32_t jn;        // 1: the previous level narrowed this row (its narrowing pass runs, low[] restarts)
    uint32_t tlow;      // keys of the source below the prefix: the sum of low[] after this level
    uint32_t pad;
};

struct TkArgs {
    const uint32_t *keys;                    // rows x cols, as the caller gave them
    uint32_t *hist;                          // [rows][TK_LEVELS][256]
    uint32_t *cnt;                           // [rows][nch][256]: each chunk's counts of the current level
    uint32_t *low, *eq, *lowbase, *eqbase;   // [rows][nch]: keys below the prefix / in the bucket, and their exclusive scans
    TkState *st;                             // [rows][TK_LEVELS + 1]
    uint32_t *cand_u, *cand_p;               // [rows][capa]
    uint32_t *surv_u, *surv_p;               // [rows][k]
    uint32_t cols, k, nch, capa, cap, xr;    // capa: cap rounded up to 64 words; xr: u = key ^ xr
};

hipError_t launch_topk_hist(const TkArgs &a, size_t rows, int level, hipStream_t s);
hipError_t launch_topk_reduce(const TkArgs &a, size_t rows, int level, hipStream_t s);
hipError_t launch_topk_scan(const TkArgs &a, size_t rows, int level, hipStream_t s);
hipError_t launch_topk_narrow(const TkArgs &a, size_t rows, int level, hipStream_t s);
hipError_t launch_topk_final(const TkArgs &a, size_t rows, hipStream_t s);
// u[i] = keys[i] ^ xr (u may be nullptr), pos[i] = i % cols
hipError_t launch_topk_prep(const uint32_t *keys, uint32_t *u, uint32_t *pos, size_t n, size_t cols, uint32_t xr,
                            hipStream_t s);
// off[i] = i * m, i <= rows
hipError_t launch_topk_offsets(uint32_t *off, size_t rows, size_t m, hipStream_t s);
// hdr[0] |= any of inner[0 .. nw) set
hipError_t launch_topk_err_acc(uint32_t *hdr, const uint32_t *inner, int nw, hipStream_t s);
// keys_out[r][j] = su[r * m + j] ^ xr, idx_out[r][j] = sp[r * m + j] for j < k (idx_out may be nullptr)
hipError_t launch_topk_write(const uint32_t *su, const uint32_t *sp, uint32_t *keys_out, uint32_t *idx_out, size_t rows,
                             size_t m, size_t k, uint32_t xr, hipStream_t s);

}  // namespace labsort
