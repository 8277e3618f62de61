// segsort.h -- segmented sort (segsort.hip): shapes, workspace header and what top-k shares of it.
#pragma once
#include <type_traits>

#include "common.h"

namespace labsort {

// ---- LDS classes: a segment is read once, sorted in LDS, written once ----
// wave classes: one wave64 per segment, no workgroup barrier; 4, 8 and 16 keys per lane for
// segments up to 256, 512 and 1024 keys.  Class-edge sweep at 2^28 keys (DESIGN.md §3.6,
// profiles/segsort_bench.txt): rows of 384 / 512 / 768 / 1024 keys took 5.2 / 4.0 / 2.9 / 2.3 ms
// in the block class and 1.45 / 1.27 / 1.17 / 1.05 ms in a wave class; one wave kernel with 8
// (16) keys per lane for every length was 5-8 % slower at 64-256 keys (15 % at 384-512) than
// the kernel with just enough registers, hence three instantiations.
#ifndef LABSORT_SEG_WAVE_KPT
#define LABSORT_SEG_WAVE_KPT 4  // A/B build knobs of the sweep
#endif
#ifndef LABSORT_SEG_WAVE2_KPT
#define LABSORT_SEG_WAVE2_KPT 8
#endif
#ifndef LABSORT_SEG_WAVE3_KPT
#define LABSORT_SEG_WAVE3_KPT 16
#endif
constexpr int SEG_WAVE_KPT = LABSORT_SEG_WAVE_KPT, SEG_WAVE2_KPT = LABSORT_SEG_WAVE2_KPT,
              SEG_WAVE3_KPT = LABSORT_SEG_WAVE3_KPT;
// longest segment of each wave class
constexpr int SEG_WAVE_KEYS = WAVE * SEG_WAVE_KPT, SEG_WAVE2_KEYS = WAVE * SEG_WAVE2_KPT,
              SEG_WAVE3_KEYS = WAVE * SEG_WAVE3_KPT;
static_assert(SEG_WAVE_KEYS < SEG_WAVE2_KEYS && SEG_WAVE2_KEYS < SEG_WAVE3_KEYS, "class edges ascend");
constexpr int SEG_WAVE_WPB = 4;  // segments (waves) per workgroup
// block class: one 256-thread workgroup per segment, 16 keys per thread
#ifndef LABSORT_SEG_BLOCK
#define LABSORT_SEG_BLOCK 256  // A/B build knobs of the hybrid finish probe
#endif
#ifndef LABSORT_SEG_BLOCK_KPT
#define LABSORT_SEG_BLOCK_KPT 16
#endif
#ifndef LABSORT_SEG_BLOCK_WGS
#define LABSORT_SEG_BLOCK_WGS 6  // keys-only grid: workgroups per CU
#endif
#ifndef LABSORT_SEG_BLOCK_WPE
#define LABSORT_SEG_BLOCK_WPE 4  // block class: waves per SIMD the register budget allows
#endif
constexpr int SEG_BLOCK_WPE = LABSORT_SEG_BLOCK_WPE;
constexpr int SEG_BLOCK = LABSORT_SEG_BLOCK;
constexpr int SEG_BLOCK_KPT = LABSORT_SEG_BLOCK_KPT;
constexpr int SEG_BLOCK_WGS = LABSORT_SEG_BLOCK_WGS;
constexpr int SEG_BLOCK_KEYS = SEG_BLOCK * SEG_BLOCK_KPT;  // 4096
// tile class: k_tile_sort's shapes, 1024 threads x 32 keys or x 16 pairs
constexpr int SEG_TILE_KEYS = TS_BLOCK * TS_KPT;        // 32768
constexpr int SEG_TILE_PAIRS = TS_BLOCK * TS_KPT_KV;    // 16384
constexpr int SEG_CLASSES = 5;
struct SegEdges {
    uint32_t e[SEG_CLASSES - 1];  // upper length bounds below the tile
};
static_assert(SEG_WAVE3_KEYS < SEG_BLOCK_KEYS, "class edges ascend");
// The class table of the segmented sort's and the dense row sort's launches: the kernel shape of class
// c (0-2 wave, 3 block, 4 tile) and its fixed grid, a multiple of the CU count: what stays resident by LDS.
struct SegClass {
    int keys;          // longest unit below the tile class (the tile's bound depends on keys / pairs)
    int block;         // threads per workgroup
    int kpt, kpt_kv;   // keys per thread: keys only, pairs
    int wpe;           // waves per SIMD in the launch bounds (block and tile kernels)
    int wgs, wgs_kv;   // workgroups per CU: keys only, pairs
};
constexpr SegClass SEG_CLASS[SEG_CLASSES] = {
    {SEG_WAVE_KEYS, SEG_WAVE_WPB * WAVE, SEG_WAVE_KPT, SEG_WAVE_KPT, 0, 8, 8},
    {SEG_WAVE2_KEYS, SEG_WAVE_WPB * WAVE, SEG_WAVE2_KPT, SEG_WAVE2_KPT, 0, 8, 6},
    {SEG_WAVE3_KEYS, SEG_WAVE_WPB * WAVE, SEG_WAVE3_KPT, SEG_WAVE3_KPT, 0, 4, 4},  // 110-127 VGPRs: four waves per SIMD
    {SEG_BLOCK_KEYS, SEG_BLOCK, SEG_BLOCK_KPT, SEG_BLOCK_KPT, SEG_BLOCK_WPE, SEG_BLOCK_WGS, 4},
    {SEG_TILE_KEYS, TS_BLOCK, TS_KPT, TS_KPT_KV, 4, 1, 1},
};
// The class of a length: the first whose edge holds it, else the tile.
inline int seg_class_of(size_t len) {
    int c = 0;
    while (c < SEG_CLASSES - 1 && len > (size_t)SEG_CLASS[c].keys) ++c;
    return c;
}
// fn(std::integral_constant<int, c>): the class as a compile-time constant, so fn names kernels by SEG_CLASS[c]
template <int C = 0, class Fn>
hipError_t seg_class_dispatch(int c, Fn &&fn) {
    if constexpr (C < SEG_CLASSES) return c == C ? fn(std::integral_constant<int, C>{}) : seg_class_dispatch<C + 1>(c, fn);
    else return hipErrorInvalidValue;
}

// Workspace header (the first 256 bytes, cleared at the start of every call).
//   word 0: offsets rejected by k_seg_bin (labsort_segments_workspace_status: ERR_ARG)
//   word 1: an inner pair sort of the general path reported an error (ERR_DEVICE)
//   words 4..8: entries in the class lists
//   word 9: the hybrid radix finish's ticket, the next grant of its block class's list (fin_block.h)
constexpr int SEG_HDR_BYTES = 256;
constexpr int SEG_HDR_DEVERR = 1, SEG_HDR_CNT = 4, SEG_HDR_TICKET = SEG_HDR_CNT + SEG_CLASSES;
static_assert((SEG_HDR_TICKET + 1) * 4 <= SEG_HDR_BYTES, "the ticket lies inside the cleared header");

// Validate the offsets (ends, monotonicity, every length <= max_len when max_len != 0) and,
// with lists != nullptr, append each segment to the list of its class (lists + c * stride).
// copy1: out of place, so 1-key segments are listed too (wave class) and get copied.
hipError_t launch_seg_bin(const uint32_t *off, size_t nseg, size_t n, size_t max_len, bool pairs, bool copy1,
                          uint32_t *hdr, uint32_t *lists, size_t stride, hipStream_t s);
// The LDS path's sort launches: the kernel of every class that max_len admits, each over its list
// (lists + c * stride).  Host arguments only: the launch sequence is fixed.  vin/vout nullptr: keys only.
// f32: the keys are float32 words, ordered by (f32_ord(key) ^ flip) and written back as words.
hipError_t launch_seg_lds_classes(size_t max_len, bool pairs, const uint32_t *in, uint32_t *out, const uint32_t *vin,
                                  uint32_t *vout, const uint32_t *off, const uint32_t *hdr, const uint32_t *lists,
                                  size_t stride, uint32_t flip, bool f32, hipStream_t s);
// ---- the hybrid radix sort's finish (api.hip's sort_radix8) ----
// After the scatter passes on digits 2 and 3 every bucket of the top 16 bits is a contiguous
// range; the finish finds the 65537 bucket offsets and sorts each bucket with the class kernels
// above, through class lists and a header of its own in the radix workspace.  Its kernels read
// the plan's choice first and return at once when the classic path was chosen.
struct HySel {
    const Plan *plan;        // nullptr: the segmented sort's own launches
    const uint32_t *buf[3];  // IN, OUT, TMP: the input is buf[plan->fin_src]
};
// finish classes: the three wave classes, a 256 x 20 block class that holds the 4096 +- 300-key
// buckets of 2^28 uniform keys (a 4096-key edge would send half of them to the tile class:
// 2.07 ms against 0.69, profiles/hybrid_finish_shapes.txt), the tile class.  (Binning every bucket
// up to 5120 keys into the block class and dropping the three wave launches saves their ~14 us on
// uniform keys, but 49152 buckets of ~4 keys beside 16384 of ~16K took 2.60 ms against 2.32: kept.)
constexpr int HY_BLOCK = 256, HY_BLOCK_KPT = 20, HY_BLOCK_WPE = 5, HY_BLOCK_KEYS = HY_BLOCK * HY_BLOCK_KPT;  // 5120
static_assert((uint32_t)SEG_TILE_KEYS == HY_MAX_BUCKET, "the plan's bound is the tile class's capacity");
static_assert(SEG_WAVE3_KEYS < HY_BLOCK_KEYS && HY_BLOCK_KEYS < SEG_TILE_KEYS, "class edges ascend");
static_assert(HY_FAST_GROUP == 4u * HY_BLOCK_KEYS, "the default gate's group bound: four block-class buckets");
// hdr: SEG_HDR_BYTES cleared since the last finish; off: HY_BUCKETS + 1 words; lists: SEG_CLASSES
// lists of HY_BUCKETS words.  Bucket offsets, class lists, the five class kernels: seven
// launches, host arguments only.  The offsets come from what the digit-3 pass left: hist, the four
// digits' totals (k_plan8's hist_out); sp3 and lookback3, that pass's SegPlan and look-back region
// of nslots slots; err, the radix workspace's error word, set when that region is unfinished.
hipError_t launch_hybrid_finish(const Plan *plan, Bufs b, size_t n, uint32_t flip, const uint32_t *hist, const SegPlan *sp3,
                                const uint32_t *lookback3, size_t nslots, uint32_t *err, uint32_t *hdr, uint32_t *off,
                                uint32_t *lists, hipStream_t s);

// workspace of the general path's inner pair sorts of n pairs (top-k's single-row sort uses the same)
size_t seg_inner_bytes(size_t n);

}  // namespace labsort
