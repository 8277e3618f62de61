// chunk_pass.h -- one stable 8-bit digit pass over rows cut into chunks of up to CHUNK consecutive
// keys, as three launches none of which waits on another workgroup, written once for the long rows
// of sort16.hip (2-byte keys) and sort64.hip (8-byte keys, passes gated by a plan): count (one
// workgroup per (row, chunk) stores its 256 digit counts to cnt[row][digit][chunk], plain stores),
// scan (exclusive, in place along the chunk axis of every (row, digit), and the row's totals
// tot[row][digit]) and scatter (one workgroup per (row, chunk): digit bases from the totals, keys
// ranked stably by digit and reordered in LDS so that a digit's run leaves as consecutive
// elements).  The kernels keep their loads, their count loops and what they store; here are the
// table and its scan, the geometry of a (row, chunk) workgroup, the scatter's digit bases, the rank
// / fold / reorder of keys held in registers (k_s64_row's passes too) and the store addresses.
#pragma once
#include <type_traits>

#include "devutil.h"
#include "host.h"

namespace labsort {

constexpr int CP_SLOTS = 32;  // LDS counter replicas per digit in the count kernels: one per bank, as k_tk_hist
// The scan along the chunk axis of the count table: up to CP_SCAN_SERIAL chunks per row one thread
// per (row, digit) walks its run of the table; above, one workgroup per (row, digit) scans it in
// steps of CP_SCAN_BLOCK chunks.
constexpr uint32_t CP_SCAN_SERIAL = 64;
constexpr int CP_SCAN_BLOCK = 1024;

// ---- the table (counts, after the scan the exclusive sums along the chunks) and the totals, in a workspace
struct ChunkTable {
    size_t off_cnt, off_tot;
};
inline ChunkTable carve_chunk_table(Carver &c, size_t rows, size_t nch) {
    const size_t cnt = c.take(rows * 256 * nch * sizeof(uint32_t));
    return {cnt, c.take(rows * 256 * sizeof(uint32_t))};
}

// ---- the chunk of a (row, chunk) workgroup of a grid of rows * nch: its first column beg and its
// length n = 1 .. CHUNK; rowoff: the row's first element
struct Chunk {
    uint32_t row, chunk, beg, n;
    size_t rowoff;
};
template <int CHUNK>
__device__ __forceinline__ Chunk chunk_of(uint32_t cols, uint32_t nch) {
    const uint32_t row = blockIdx.x / nch, chunk = blockIdx.x - row * nch, beg = chunk * (uint32_t)CHUNK;
    return {row, chunk, beg, cols - beg > (uint32_t)CHUNK ? (uint32_t)CHUNK : cols - beg, (size_t)row * cols};
}
// where the chunk's count of digit d stands in the table
__device__ __forceinline__ size_t chunk_cnt_at(const Chunk &c, uint32_t d, uint32_t nch) {
    return ((size_t)c.row * 256u + d) * nch + c.chunk;
}

// ---- scan.  Gate: a callable, uniform over the grid, that says whether the pass runs at all
struct AlwaysOn {  // (no load and no branch)
    __device__ __forceinline__ bool operator()() const { return true; }
};

namespace {  // (the kernels are each including file's own)

// few chunks per row: thread i walks the nch words of (row, digit) i = row * 256 + digit
template <class Gate>
__global__ __launch_bounds__(256) void k_chunk_scan_serial(uint32_t *cnt, uint32_t *tot, uint32_t nrd, uint32_t nch, Gate on) {
    if (!on()) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nrd) return;
    uint32_t *p = cnt + (size_t)i * nch;
    uint32_t run = 0u;
    for (uint32_t c = 0; c < nch; ++c) {
        const uint32_t t = p[c];
        p[c] = run;
        run += t;
    }
    tot[i] = run;
}

// many chunks per row: workgroup i scans the nch words of (row, digit) i in steps of its width
template <class Gate>
__global__ __launch_bounds__(CP_SCAN_BLOCK) void k_chunk_scan_block(uint32_t *cnt, uint32_t *tot, uint32_t nch, Gate on) {
    if (!on()) return;
    constexpr int NW = CP_SCAN_BLOCK / WAVE;
    __shared__ uint32_t wsum[NW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t *p = cnt + (size_t)blockIdx.x * nch;
    uint32_t carry = 0u;
    for (uint32_t c0 = 0; c0 < nch; c0 += (uint32_t)CP_SCAN_BLOCK) {  // (uniform over the workgroup)
        const uint32_t c = c0 + tid;
        const uint32_t v = c < nch ? p[c] : 0u;
        const uint32_t x = wave_incl_scan(v, lane);
        if (lane == 63u) wsum[wid] = x;
        __syncthreads();
        uint32_t add = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t t = wsum[w];
            if ((uint32_t)w < wid) add += t;
            total += t;
        }
        if (c < nch) p[c] = carry + add + x - v;
        carry += total;
        __syncthreads();  // (wsum is written again in the next step)
    }
    if (tid == 0u) tot[blockIdx.x] = carry;
}

// the scan of a pass over rows x nch chunks: one launch, chosen by the chunks per row
template <class Gate>
inline void launch_chunk_scan(uint32_t *cnt, uint32_t *tot, size_t rows, uint32_t nch, Gate on, hipStream_t s) {
    const uint32_t nrd = (uint32_t)(rows * 256);
    if (nch <= CP_SCAN_SERIAL) k_chunk_scan_serial<<<(nrd + 255u) / 256u, 256, 0, s>>>(cnt, tot, nrd, nch, on);
    else k_chunk_scan_block<<<nrd, CP_SCAN_BLOCK, 0, s>>>(cnt, tot, nch, on);
}

}  // namespace

// ---- scatter.  Digit d = tid < 256: the row element that this chunk's first key of digit d goes
// to, from the row's totals and what the chunks before this one hold of d.  Must be called by
// every thread (contains a barrier).
template <int BLOCK>
__device__ __forceinline__ uint32_t chunk_digit_base(const uint32_t *cnt, const uint32_t *tot, const Chunk &c, uint32_t nch,
                                                     uint32_t *wsum) {
    const uint32_t tid = threadIdx.x;
    uint32_t t = 0u, pre = 0u;
    if (tid < 256u) {
        t = tot[(size_t)c.row * 256u + tid];
        pre = cnt[chunk_cnt_at(c, tid, nch)];
    }
    return block_excl_scan<BLOCK, 256>(t, wsum) + pre;
}

// ---- the digit pass over up to BLOCK * KPT keys in registers.  Wave wid holds slots ws0 ..
// ws0 + 64 * KPT - 1, slot ws0 + j * 64 + lane in k[j]: in order of position over (wave, j, lane).
// Slots from n on are padding, all ones: digit 255 in every pass and behind every key, so the
// first n slots of the digit order hold the keys.  K: uint32_t (a 16-bit image) or uint64_t.
template <class K>
__device__ __forceinline__ uint32_t digit_of(K u, uint32_t shift) {
    return (uint32_t)(u >> shift) & 0xFFu;
}
template <int KPT>
struct WaveStripe {
    uint32_t ws0, ng;  // the first slot; the 64-key groups of this wave that hold keys (wave-uniform)
    __device__ __forceinline__ WaveStripe(uint32_t wid, uint32_t n) : ws0(wid * (uint32_t)(WAVE * KPT)) {
        ng = ws0 < n ? (n - ws0 + 63u) / 64u : 0u;
        if (ng > (uint32_t)KPT) ng = KPT;
    }
    __device__ __forceinline__ uint32_t slot(int j, uint32_t lane) const { return ws0 + (uint32_t)j * WAVE + lane; }
};

// Zeroes the wave's counters, ranks its keys stably by the digit at `shift` (the lane-ordered wave
// ranking of devutil.h) into packed 16-bit wave-local ranks, and behind a barrier (every wave's
// counters are complete; the caller's reads of the LDS keys are done) folds the counters to first
// slots.  The caller's barrier follows.  Must be called by every thread.
template <int BLOCK, int KPT, class K>
__device__ __forceinline__ DigitSpan chunk_rank(const K (&k)[KPT], uint32_t shift, uint32_t ng, uint32_t *whist, uint32_t *wsum,
                                                uint32_t (&rank)[KPT / 2], bool atomic_rank, uint32_t lane, uint32_t wid) {
    static_assert(KPT % 2 == 0 && BLOCK % 256 == 0, "ranks are packed in pairs; 256 threads hold the digits");
    static_assert(BLOCK * KPT <= 65536, "a rank, a slot and a key's place in its row or chunk are 16 bits");
    uint32_t *wh = whist + wid * 256u;
    for (uint32_t i = lane; i < 256u; i += WAVE) wh[i] = 0u;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        uint32_t r = 0u;
        if ((uint32_t)j < ng) r = rank8(wh, digit_of(k[j], shift), lane, atomic_rank);
        set16(rank, j, r);
    }
    __syncthreads();
    return fold_digit_offsets<BLOCK, BLOCK / WAVE>(whist, wsum);
}

// What a key carries through LDS beside itself: C = uint16_t (its place), uint32_t (its position)
// or NoCarry.
struct NoCarry {};
// Keys k, and v as C, into their slots of the digit order.  Ranked slots number the keys and the
// padding of the last group: dst < BLOCK * KPT.  The caller's barrier follows.  AHEAD: every
// destination first (replacing its 16-bit rank), the stores after, as lds_pass.h does and says why
// (the 2-byte keys); else each key's counter read right before its stores (the 8-byte keys, whose
// k_s64_row measured 2 % slower in the first form in two sessions).
template <bool AHEAD, int KPT, class K, class KS, class C, int NV>
__device__ __forceinline__ void chunk_reorder(const K (&k)[KPT], const uint32_t (&v)[NV], uint32_t shift, uint32_t ng,
                                              const uint32_t *wh, uint32_t (&rank)[KPT / 2], KS *keys, C *pay) {
    constexpr bool CARRY = !std::is_same<C, NoCarry>::value;
    static_assert(!CARRY || NV == KPT, "one carried value per key");
    if constexpr (AHEAD) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) set16(rank, j, wh[digit_of(k[j], shift)] + get16(rank, j));
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if ((uint32_t)j < ng) {
            const uint32_t dst = AHEAD ? get16(rank, j) : wh[digit_of(k[j], shift)] + get16(rank, j);
            keys[dst] = (KS)k[j];
            if constexpr (CARRY) pay[dst] = (C)v[j];
        }
}

// The scatter's stores: slot i of the digit order goes to row element o = goff[digit] + i, so
// consecutive slots of one digit are consecutive elements of the row; store(i, u, o) writes it.
template <int BLOCK, class KS, class Store>
__device__ __forceinline__ void chunk_store(const KS *keys, const uint32_t *goff, uint32_t shift, uint32_t n, uint32_t cols,
                                            Store store) {
    for (uint32_t i = threadIdx.x; i < n; i += BLOCK) {
        const KS u = keys[i];
        const uint32_t o = goff[digit_of(u, shift)] + i;
        if (o >= cols) continue;  // (cannot happen while the count and the scatter read the same keys)
        store(i, u, o);
    }
}

}  // namespace labsort
