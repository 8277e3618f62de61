// kth.hip -- k-th key selection per row (labsort_kth_device): which key is the k-th of every row
// of a dense matrix, and where it is; k is one host value or one word per row in device memory.
// All kernels work on u, where plain uint32 order is the order asked for (topk.hip's images):
//   int32 / uint32   u = key ^ xr
//   float32          u = f32_ord(key) ^ xr
//   bfloat16/float16 u = (ord16(key) << 16) ^ xr, xr = largest ? 0xFFFF0000 : 0; two digit levels
// The MSD radix select with 8-bit digits of topk.hip, stopped at the threshold: after the last
// level the prefix is the k-th key and krem its rank among its ties.  No survivor list, no
// candidate buffer, no inner sort, no scatter.
//
// Rows of up to KTH_ROW_KEYS keys: k_kth_short, one launch, one workgroup per row (256 threads up to
// KTH_SMALL_ROW_KEYS keys, 1024 above).  The row is loaded once as u and held in registers; every
// level counts into the slotted LDS histogram and every wave picks the same digit from it; the
// position comes from one ordered block scan of the keys equal to the threshold.
// Longer rows are cut into chunks of TK_CHUNK keys; per level
//   k_kth_hist  counts the level's digit of the keys that match the prefix, per chunk (cnt, plain
//               stores) and per row (hist, one atomic add per workgroup and digit).  From level 1
//               on a chunk is read only if it held a key of the digit chosen at the level before
//               (one word of its own row of cnt, read before the row is overwritten); a skipped
//               chunk's row of cnt is zeroed, so that no later level takes stale counts for keys.
//   k_kth_pick  one workgroup per row: the digit at which the running count reaches krem, and
//               the next level's state.  Level 0 reads and validates the row's k.  After the last
//               level: without positions it writes the key; with them it scans cnt[row][*][digit]
//               along the chunks for the chunk that holds the krem-th tie and the rank within it.
//   k_kth_locate  (with positions) one workgroup per row reads that one chunk in position order
//               and writes the key and the position.
// Every dependency between workgroups is a kernel boundary: no kernel waits on another workgroup.
//
// Top-k filtering (labsort_topk_mask_device) applies the threshold: the row written back with the
// first k of its (u, position) pairs kept and the fill elsewhere, and / or their mask.
//   k_kth_short<.., FILTER = true>  rows of up to KTH_ROW_KEYS keys, one launch: the same kernel
//                template, so the load and the level loop stand once; after the select the
//                threshold's ties are ranked in position order and every thread stores the groups
//                it holds.  There is no kernel of the filter's own name: a profiler lists the
//                select as k_kth_short<KT, BLOCK, SLOTS, false> and the filter as <.., true>.
//   k_tkm_apply  longer rows, after the launches above with positions: one workgroup per (row,
//                chunk) tests every key against the row's k-th pair and stores.
// Both instantiations compile to the text the two separate kernels had.
//
// Top-p filtering (labsort_top_p_device) is the same select on masses: every key weighs
// min(floor(x 2^40), 2^40), the level histograms hold 64-bit sums of weights, and the digit picked is
// the one at which the running mass reaches the row's target.
//   k_tp_short   rows of up to KTH_ROW_KEYS keys, one launch: the mass select with the row in
//                registers, then the filter's ordered scan of the threshold's ties and its stores.
//   k_tp_hist / k_tp_pick  longer rows, per level, in the shape of k_kth_hist / k_kth_pick; the last
//                pick writes the KthState that k_kth_locate and k_tkm_apply read, and those two run
//                as they do for the top-k filter (k_tkm_apply<.., COUNT = true> also counts what it
//                keeps, for the call's kept-count output).
//
// Categorical sampling (labsort_sample_device) draws positions by inverse CDF on the same weights: a
// prefix sum in position order and a search for where it crosses floor(U W / 2^32).
//   k_smp_short  rows of up to KTH_ROW_KEYS keys, one launch: the row in registers, one ordered 64-bit
//                scan of the groups' masses, then every draw of the row by the thread whose group holds it.
//   k_smp_sum / k_smp_pick / k_smp_locate  longer rows: each chunk's mass; per row the prefix of the
//                chunk masses and per draw its chunk and what is left of the target; per (row, draw)
//                that one chunk searched as k_smp_short searches a row.
#include "kth.h"

#include <type_traits>

#include "devutil.h"
#include "host.h"

namespace labsort {

// Per row and level: what the level's kernels read.  Level L's pick writes entry L + 1, so no
// kernel reads a word that another workgroup of the same launch writes.
struct KthState {
    uint32_t prefix;  // digits chosen so far, in place (the top 8 * level bits)
    uint32_t krem;    // rank of the k-th key among the keys that match the prefix (>= 1)
    uint32_t d;       // the digit chosen at the level before: a chunk without such a key is skipped
    uint32_t cstar;   // entry `levels` only: the chunk that holds the krem-th key equal to prefix (krem: within it)
};

struct KthArgs {
    const void *keys;     // rows x cols, as the caller gave them (16-bit key types: 2-byte elements)
    const uint32_t *d_k;  // [rows], or nullptr: k
    uint32_t *hdr;        // word 0: a row's k was out of range
    uint32_t *hist;       // [rows][TK_LEVELS][256]
    uint32_t *cnt;        // [rows][nch][256]: each chunk's counts of the current level
    KthState *st;         // [rows][TK_LEVELS + 1]
    void *keys_out;       // [rows]
    uint32_t *idx_out;    // [rows], or nullptr
    uint32_t cols, k, nch, xr;
};

namespace {

enum KthKey : int { KTH_INT, KTH_F32, KTH_BF16, KTH_F16 };
constexpr bool kth_is16(int kt) { return kt == KTH_BF16 || kt == KTH_F16; }
constexpr uint32_t kth_nan_t(int kt) { return kt == KTH_BF16 ? BF16_NAN_T : F16_NAN_T; }
constexpr int kth_levels(int kt) { return kth_is16(kt) ? 2 : TK_LEVELS; }
template <int KT>
using kth_elem_t = std::conditional_t<kth_is16(KT), uint16_t, uint32_t>;
template <int KT>
constexpr int KTH_E = 16 / (int)sizeof(kth_elem_t<KT>);  // keys per 16-byte load

// u of an element x of the input (ord16 reads the low half of x), and the key of an image
template <int KT>
__device__ __forceinline__ uint32_t kth_u(uint32_t x, uint32_t xr) {
    if constexpr (kth_is16(KT)) return (ord16(x, kth_nan_t(KT)) << 16) ^ xr;
    else if constexpr (KT == KTH_F32) return f32_ord(x) ^ xr;
    else return x ^ xr;
}
__device__ __forceinline__ void kth_write_key(void *keys_out, uint32_t row, uint32_t u, uint32_t xr, int kt) {
    const uint32_t w = u ^ xr;
    if (kth_is16(kt)) static_cast<uint16_t *>(keys_out)[row] = (uint16_t)unord16(w >> 16);  // (either format)
    else static_cast<uint32_t *>(keys_out)[row] = kt == KTH_F32 ? f32_unord(w) : w;
}
template <int KT>
__device__ __forceinline__ const kth_elem_t<KT> *kth_row(const KthArgs &a, uint32_t row) {
    return static_cast<const kth_elem_t<KT> *>(a.keys) + (size_t)row * a.cols;
}
// Group q of [beg, end) of a row as u (devutil.h, load_group)
template <int KT>
__device__ __forceinline__ uint32_t kth_load(const kth_elem_t<KT> *base, uint32_t beg, uint32_t end, uint32_t mis, uint32_t q,
                                             uint32_t xr, uint32_t (&u)[KTH_E<KT>], int64_t &i0) {
    return load_group(base, beg, end, mis, q, u, i0, [xr](uint32_t x) { return kth_u<KT>(x, xr); });
}
// Chunk c of a long row: its keys [beg, end) and their groups (devutil.h, group_mis / group_count)
struct KthChunk {
    uint32_t beg, end, mis, nq;
};
template <int KT>
__device__ __forceinline__ KthChunk kth_chunk(const kth_elem_t<KT> *base, uint32_t cols, uint32_t c) {
    KthChunk ch;
    ch.beg = c * TK_CHUNK;
    ch.end = cols - ch.beg > (uint32_t)TK_CHUNK ? ch.beg + TK_CHUNK : cols;
    ch.mis = group_mis(base, ch.beg);
    ch.nq = group_count<KTH_E<KT>>(ch.beg, ch.end, ch.mis);
    return ch;
}

// The row's k, clamped into [1, cols]; a k outside is reported in the header by the thread told to
__device__ __forceinline__ uint32_t kth_k(const KthArgs &a, uint32_t row, bool report) {
    const uint32_t kk = a.d_k ? a.d_k[row] : a.k;
    if (kk >= 1u && kk <= a.cols) return kk;
    if (report) a.hdr[0] = 1u;
    return kk < 1u ? 1u : a.cols;
}

// The digit at which the running count of a level histogram (256 words, 16-byte aligned, global or
// LDS) reaches krem: the d with count(< d) < krem <= count(<= d), topk.hip's rule (tk_pick, which
// stays in its translation unit: moving it to a header would rebuild topk.hip's kernels, DESIGN.md
// §3.15).  Called by a whole wave; the result is wave-uniform.
struct KthPick {
    uint32_t d, below;
};
__device__ __forceinline__ KthPick kth_pick(const uint32_t *hrow, uint32_t krem, uint32_t lane) {
    const uint4 v = reinterpret_cast<const uint4 *>(hrow)[lane];  // digits 4 lane .. 4 lane + 3
    const uint32_t c[4] = {v.x, v.y, v.z, v.w};
    const uint32_t s = v.x + v.y + v.z + v.w;
    const uint32_t x = wave_incl_scan(s, lane);
    uint32_t run = x - s, d = 255u, below = x - c[3];  // (lane 63's default: the last digit)
    bool found = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!found && run < krem && krem <= run + c[j]) {
            found = true;
            d = 4u * lane + (uint32_t)j;
            below = run;
        }
        run += c[j];
    }
    const uint64_t m = __ballot(found);
    const int srcl = m ? __ffsll((long long)m) - 1 : 63;  // (no lane: krem exceeds the row's count, which cannot happen)
    KthPick p;
    p.d = __shfl(d, srcl);
    p.below = __shfl(below, srcl);
    if (p.below >= krem) p.below = krem - 1u;  // keeps krem >= 1 whatever the histogram held
    return p;
}

// Which of the set bits of em is the n-th (n >= 1, at most popc(em))
template <int E>
__device__ __forceinline__ uint32_t kth_nth_bit(uint32_t em, uint32_t n) {
    uint32_t seen = 0u, at = 0u;
#pragma unroll
    for (int j = 0; j < E; ++j)
        if ((em >> j) & 1u) {
            if (++seen == n) at = (uint32_t)j;
        }
    return at;
}

// One step of an ordered scan over the workgroup: thread tid holds c items, carry is the count of
// the steps before.  Returns the items before this thread's; adds the step's total to carry.
// Two barriers: wsum and tot are free again on return.
template <int BLOCK = KTH_BLOCK>
__device__ __forceinline__ uint32_t kth_ordered_step(uint32_t c, uint32_t &carry, uint32_t *wsum, uint32_t *tot) {
    const uint32_t ex = block_excl_scan<BLOCK, BLOCK>(c, wsum);
    if (threadIdx.x == BLOCK - 1u) *tot = ex + c;
    __syncthreads();
    const uint32_t before = carry + ex;
    carry += *tot;
    __syncthreads();
    return before;
}

// ---- top-k filtering (labsort_topk_mask_device): the row written back with everything outside its
// first k (u, position) pairs replaced by the fill, and / or the mask of the pairs kept ----
struct TkmArgs {
    void *keys_out;       // rows x cols elements of the key type (may be the input itself), or nullptr
    uint8_t *mask_out;    // rows x cols bytes, or nullptr
    const uint32_t *pos;  // long rows: [rows], the position of each row's k-th pair (k_kth_locate's output)
    uint32_t fill;        // what an element outside the top k becomes
};

// The key of an image, as a word of the key type (kth_write_key's transform)
template <int KT>
__device__ __forceinline__ uint32_t kth_unord(uint32_t u, uint32_t xr) {
    const uint32_t w = u ^ xr;
    if constexpr (kth_is16(KT)) return unord16(w >> 16);
    else if constexpr (KT == KTH_F32) return f32_unord(w);
    else return w;
}

// Stores one group of a row: elements i0 .. i0 + E - 1 (those of vm exist, rowoff = row * cols), w[j]
// the word of element j (its key or the fill), bit j of km set where it is kept.  A group that lies
// wholly inside the row is one 16-byte store of keys and one E-byte store of mask bytes where the
// address allows it; everything else goes element by element, so that no store covers an element
// of another row.  The keys' and the mask's alignment are tested each on its own.
template <int KT>
__device__ __forceinline__ void tkm_store(const TkmArgs &m, size_t rowoff, int64_t i0, uint32_t vm,
                                          const uint32_t (&w)[KTH_E<KT>], uint32_t km) {
    constexpr int E = KTH_E<KT>;
    constexpr uint32_t FULL = (1u << E) - 1u;
    using elem_t = kth_elem_t<KT>;
    if (m.keys_out) {
        const uintptr_t at = (uintptr_t)m.keys_out + (uintptr_t)(((int64_t)rowoff + i0) * (int64_t)sizeof(elem_t));
        if (vm == FULL && (at & 15u) == 0u) {
            uint4 v;
            if constexpr (E == 4) v = make_uint4(w[0], w[1], w[2], w[3]);
            else v = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
            *reinterpret_cast<uint4 *>(at) = v;
        } else {
#pragma unroll
            for (int j = 0; j < E; ++j)
                if ((vm >> j) & 1u) reinterpret_cast<elem_t *>(at)[j] = (elem_t)w[j];
        }
    }
    if (m.mask_out) {
        const uintptr_t at = (uintptr_t)m.mask_out + (uintptr_t)((int64_t)rowoff + i0);
        // bits 0..3 of x as four bytes of 0 / 1
        auto spread = [](uint32_t x) { return (x & 1u) | ((x & 2u) << 7) | ((x & 4u) << 14) | ((x & 8u) << 21); };
        if (vm == FULL && (at & (uintptr_t)(E - 1)) == 0u) {
            if constexpr (E == 4) *reinterpret_cast<uint32_t *>(at) = spread(km);
            else *reinterpret_cast<uint2 *>(at) = make_uint2(spread(km), spread(km >> 4));
        } else {
#pragma unroll
            for (int j = 0; j < E; ++j)
                if ((vm >> j) & 1u) reinterpret_cast<uint8_t *>(at)[j] = (uint8_t)((km >> j) & 1u);
        }
    }
}

// ---- rows of up to BLOCK * KTH_KPT keys: one workgroup of BLOCK threads, the row in registers;
// SLOTS counter replicas per digit.  FILTER = false: the select, which writes the k-th key and its
// position (m is not read).  FILTER = true: the top-k filter, which after the same select writes
// back the groups every thread holds (a.keys_out and a.idx_out are not read) ----
template <int KT, int BLOCK, int SLOTS, bool FILTER>
__global__ __launch_bounds__(BLOCK) void k_kth_short(KthArgs a, TkmArgs m) {
    constexpr int E = KTH_E<KT>, T = KTH_KPT / E;
    constexpr int TG = T + 1;  // a row that starts inside a group has one group more
    constexpr int NLEV = kth_levels(KT);
    __shared__ uint32_t h[256 * SLOTS];
    __shared__ __attribute__((aligned(16))) uint32_t hrow[256];
    __shared__ uint32_t wsum[BLOCK / WAVE], tot;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const uint32_t mis = group_mis(base, 0u), nq = group_count<E>(0u, a.cols, mis);  // <= T * BLOCK + 1
    uint32_t u[TG][E], vm[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const uint32_t q = (uint32_t)t * BLOCK + tid;
        int64_t i0;
        vm[t] = 0u;
        if (q < nq) vm[t] = kth_load<KT>(base, 0u, a.cols, mis, q, a.xr, u[t], i0);
        else
#pragma unroll
            for (int j = 0; j < E; ++j) u[t][j] = 0u;
    }
    uint32_t prefix = 0u, krem = kth_k(a, row, tid == 0u), ties = 0u;
    for (int level = 0; level < NLEV; ++level) {
        const uint32_t shift = 24u - 8u * (uint32_t)level;
        const uint32_t mask = level ? 0xFFFFFFFFu << (shift + 8u) : 0u;
        slot_hist_clear<SLOTS, BLOCK>(h, tid);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int j = 0; j < E; ++j)
                if (((vm[t] >> j) & 1u) && ((u[t][j] ^ prefix) & mask) == 0u)
                    slot_hist_add<SLOTS>(h, (u[t][j] >> shift) & 255u, tid);
        __syncthreads();
        if (tid < 256u) hrow[tid] = slot_hist_fold<SLOTS>(h, tid);
        __syncthreads();
        const KthPick p = kth_pick(hrow, krem, lane);  // (every wave: the same answer)
        prefix |= p.d << shift;
        krem -= p.below;
        // after the last level: the keys equal to the threshold (hrow stays until the next level's barriers)
        if constexpr (FILTER) ties = hrow[p.d];
    }
    if constexpr (FILTER) {
        // km[t]: the elements of group (t, tid) that are kept: the keys below the threshold and the first
        // krem of its ties in position order.  ties == krem (uniform): all of them, no scan.
        uint32_t km[TG];
        const bool all_ties = LABSORT_TKM_SKIP_SCAN && ties == krem;
        uint32_t carry = 0u;
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            uint32_t lt = 0u, em = 0u;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool v = (vm[t] >> j) & 1u;
                lt |= (v && u[t][j] < prefix ? 1u : 0u) << j;
                em |= (v && u[t][j] == prefix ? 1u : 0u) << j;
            }
            km[t] = lt;
            if (all_ties) km[t] |= em;
            else if (carry < krem) {  // (uniform; past it no tie is kept)
                const uint32_t c = (uint32_t)__popc(em);
                const uint32_t before = kth_ordered_step<BLOCK>(c, carry, wsum, &tot);
                const uint32_t room = before < krem ? krem - before : 0u;
                uint32_t seen = 0u;
#pragma unroll
                for (int j = 0; j < E; ++j)
                    if ((em >> j) & 1u) {
                        if (seen < room) km[t] |= 1u << j;
                        ++seen;
                    }
            }
        }
        const size_t rowoff = (size_t)row * a.cols;
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const uint32_t q = (uint32_t)t * BLOCK + tid;
            if (q >= nq) continue;
            uint32_t w[E];
#pragma unroll
            for (int j = 0; j < E; ++j) w[j] = (km[t] >> j) & 1u ? kth_unord<KT>(u[t][j], a.xr) : m.fill;
            tkm_store<KT>(m, rowoff, (int64_t)E * q - (int64_t)mis, vm[t], w, km[t]);
        }
        return;
    }
    if (a.idx_out) {
        // groups in position order: (t, tid); krem: the rank of the k-th key among the keys equal to prefix
        uint32_t carry = 0u;
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            if (carry >= krem) break;  // (uniform)
            uint32_t em = 0u;
#pragma unroll
            for (int j = 0; j < E; ++j) em |= (((vm[t] >> j) & 1u) && u[t][j] == prefix ? 1u : 0u) << j;
            const uint32_t c = (uint32_t)__popc(em);
            const uint32_t before = kth_ordered_step<BLOCK>(c, carry, wsum, &tot);
            if (c && before < krem && krem <= before + c) {
                const uint32_t q = (uint32_t)t * BLOCK + tid;
                a.idx_out[row] = E * q - mis + kth_nth_bit<E>(em, krem - before);
            }
        }
    }
    if (tid == 0u) kth_write_key(a.keys_out, row, prefix, a.xr, KT);
}

// ---- longer rows ----
// Workgroup bx of a row counts chunks bx g .. bx g + g - 1 (topk.hip's k_tk_hist: at most
// TK_MAX_HIST_WG workgroups add to a row's histogram).
template <int KT>
__global__ __launch_bounds__(KTH_BLOCK) void k_kth_hist(KthArgs a, int level, uint32_t nx, uint32_t g) {
    constexpr int E = KTH_E<KT>, T = KTH_KPT / E;
    __shared__ uint32_t h[256 * TK_SLOTS];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / nx, bx = blockIdx.x - row * nx;
    const uint32_t c0 = bx * g;
    if (c0 >= a.nch) return;
    const uint32_t c1 = c0 + g < a.nch ? c0 + g : a.nch;
    KthState st{0u, 0u, 0u, 0u};
    if (level) st = a.st[(size_t)row * (TK_LEVELS + 1) + level];
    const uint32_t shift = 24u - 8u * (uint32_t)level;
    const uint32_t mask = level ? 0xFFFFFFFFu << (shift + 8u) : 0u;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const uint32_t xr = a.xr, prefix = st.prefix;
    uint32_t acc = 0u;
    for (uint32_t c = c0; c < c1; ++c) {
        uint32_t *crow = a.cnt + ((size_t)row * a.nch + c) * 256u;
        // the chunk's count of the digit chosen at the level before: every thread reads the same word,
        // which within this launch only this workgroup writes, and only zero over zero before the barriers below
        if (level && __builtin_amdgcn_readfirstlane(crow[st.d]) == 0u) {
            if (tid < 256u) crow[tid] = 0u;  // (no stale counts of the level before)
            continue;
        }
        slot_hist_clear<TK_SLOTS, KTH_BLOCK>(h, tid);
        __syncthreads();
        const KthChunk ch = kth_chunk<KT>(base, a.cols, c);
        for (uint32_t q0 = 0; q0 < ch.nq; q0 += (uint32_t)T * KTH_BLOCK) {
            uint32_t u[T][E], vm[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const uint32_t q = q0 + (uint32_t)t * KTH_BLOCK + tid;
                int64_t i0;
                vm[t] = 0u;
                if (q < ch.nq) vm[t] = kth_load<KT>(base, ch.beg, ch.end, ch.mis, q, xr, u[t], i0);
                else
#pragma unroll
                    for (int j = 0; j < E; ++j) u[t][j] = 0u;
            }
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int j = 0; j < E; ++j)
                    if (((vm[t] >> j) & 1u) && ((u[t][j] ^ prefix) & mask) == 0u)
                        slot_hist_add<TK_SLOTS>(h, (u[t][j] >> shift) & 255u, tid);
        }
        __syncthreads();
        if (tid < 256u) {
            const uint32_t sum = slot_hist_fold<TK_SLOTS>(h, tid);
            crow[tid] = sum;
            acc += sum;
        }
        __syncthreads();
    }
    if (tid < 256u && acc) atomicAdd(&a.hist[((size_t)row * TK_LEVELS + level) * 256u + tid], acc);
}

// last: the call's last level.  kt: the key type, for the key a call without positions writes here.
__global__ __launch_bounds__(KTH_BLOCK) void k_kth_pick(KthArgs a, int level, int last, int kt) {
    __shared__ uint32_t wsum[KTH_BLOCK / WAVE], tot, hit[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x;
    KthState st{0u, 0u, 0u, 0u};
    if (level) st = a.st[(size_t)row * (TK_LEVELS + 1) + level];
    else st.krem = kth_k(a, row, tid == 0u);
    const KthPick p = kth_pick(a.hist + ((size_t)row * TK_LEVELS + level) * 256u, st.krem, lane);
    KthState ns;
    ns.prefix = st.prefix | (p.d << (24u - 8u * (uint32_t)level));
    ns.krem = st.krem - p.below;
    ns.d = p.d;
    ns.cstar = 0u;
    KthState *out = a.st + (size_t)row * (TK_LEVELS + 1) + level + 1;
    if (!last) {
        if (tid == 0u) *out = ns;
        return;
    }
    if (!a.idx_out) {
        if (tid == 0u) kth_write_key(a.keys_out, row, ns.prefix, a.xr, kt);
        return;
    }
    // the chunk that holds the krem-th key equal to the threshold, from the last level's counts of its
    // last digit (zero for a skipped chunk), in steps of the block size
    if (tid == 0u) {
        hit[0] = 0u;
        hit[1] = 1u;
    }
    __syncthreads();
    uint32_t carry = 0u;
    for (uint32_t b = 0; b < a.nch && carry < ns.krem; b += KTH_BLOCK) {  // (uniform)
        const uint32_t c = b + tid;
        const uint32_t v = c < a.nch ? a.cnt[((size_t)row * a.nch + c) * 256u + p.d] : 0u;
        const uint32_t before = kth_ordered_step(v, carry, wsum, &tot);
        if (v && before < ns.krem && ns.krem <= before + v) {
            hit[0] = c;
            hit[1] = ns.krem - before;
        }
    }
    __syncthreads();
    if (tid == 0u) {
        ns.cstar = hit[0];
        ns.krem = hit[1];
        *out = ns;
    }
}

template <int KT>
__global__ __launch_bounds__(KTH_BLOCK) void k_kth_locate(KthArgs a) {
    constexpr int E = KTH_E<KT>;
    __shared__ uint32_t wsum[KTH_BLOCK / WAVE], tot;
    const uint32_t tid = threadIdx.x, row = blockIdx.x;
    const KthState st = a.st[(size_t)row * (TK_LEVELS + 1) + kth_levels(KT)];
    const uint32_t c = st.cstar < a.nch ? st.cstar : a.nch - 1u;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const KthChunk ch = kth_chunk<KT>(base, a.cols, c);
    uint32_t carry = 0u;
    for (uint32_t q0 = 0; q0 < ch.nq && carry < st.krem; q0 += KTH_BLOCK) {  // (uniform)
        const uint32_t q = q0 + tid;
        uint32_t u[E], vm = 0u;
        int64_t i0 = 0;
        if (q < ch.nq) vm = kth_load<KT>(base, ch.beg, ch.end, ch.mis, q, a.xr, u, i0);
        uint32_t em = 0u;
#pragma unroll
        for (int j = 0; j < E; ++j) em |= (((vm >> j) & 1u) && u[j] == st.prefix ? 1u : 0u) << j;
        const uint32_t n = (uint32_t)__popc(em);
        const uint32_t before = kth_ordered_step(n, carry, wsum, &tot);
        if (n && before < st.krem && st.krem <= before + n)
            a.idx_out[row] = (uint32_t)i0 + kth_nth_bit<E>(em, st.krem - before);  // (a set bit: inside [beg, end))
    }
    if (tid == 0u) kth_write_key(a.keys_out, row, st.prefix, a.xr, KT);
}

// The filter's longer rows, after the select with positions: one workgroup per (row, chunk) streams
// its chunk through the test against the row's k-th pair (uT, P).  COUNT (top-p filtering, where
// the number kept is a result): the elements kept are counted and added to kept[row], which is
// zero before the launch, once per workgroup; either output of m may then be absent.
template <int KT, bool COUNT>
__global__ __launch_bounds__(KTH_BLOCK) void k_tkm_apply(KthArgs a, TkmArgs m, uint32_t *kept) {
    constexpr int E = KTH_E<KT>, T = KTH_KPT / E;
    __shared__ uint32_t nkept;
    const uint32_t tid = threadIdx.x;
    uint32_t mine = 0u;
    if constexpr (COUNT) {
        if (tid == 0u) nkept = 0u;
        __syncthreads();
    }
    const uint32_t row = blockIdx.x / a.nch, c = blockIdx.x - row * a.nch;
    const uint32_t uT = a.st[(size_t)row * (TK_LEVELS + 1) + kth_levels(KT)].prefix, P = m.pos[row];
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const size_t rowoff = (size_t)row * a.cols;
    const KthChunk ch = kth_chunk<KT>(base, a.cols, c);
    for (uint32_t q0 = 0; q0 < ch.nq; q0 += (uint32_t)T * KTH_BLOCK) {
        uint32_t u[T][E], vm[T];
        int64_t i0[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t q = q0 + (uint32_t)t * KTH_BLOCK + tid;
            vm[t] = 0u;
            i0[t] = 0;
            if (q < ch.nq) vm[t] = kth_load<KT>(base, ch.beg, ch.end, ch.mis, q, a.xr, u[t], i0[t]);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (!vm[t]) continue;
            uint32_t w[E], km = 0u;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool keep = ((vm[t] >> j) & 1u) && (u[t][j] < uT || (u[t][j] == uT && i0[t] + j <= (int64_t)P));
                km |= (keep ? 1u : 0u) << j;
                w[j] = keep ? kth_unord<KT>(u[t][j], a.xr) : m.fill;
            }
            tkm_store<KT>(m, rowoff, i0[t], vm[t], w, km);
            if constexpr (COUNT) mine += (uint32_t)__popc(km);
        }
    }
    if constexpr (COUNT) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if ((tid & 63u) == 0u && mine) atomicAdd(&nkept, mine);
        __syncthreads();
        if (tid == 0u && nkept) atomicAdd(&kept[row], nkept);
    }
}

// ---- top-p filtering (labsort_top_p_device): the select above with masses for counts.  An
// element weighs w = min(floor(x 2^40), 2^40), zero for a set sign bit and for a NaN; a row's
// target is t = max(1, ceil(P W / 2^32)) with W its total and P = clamp(floor(p 2^32), 1, 2^32).
// Every level sums the weights of the keys that match the prefix by digit and picks the digit at
// which the running mass reaches what is left of t.  The last prefix is the threshold T, w(T) > 0,
// and the first ceil(trem / w(T)) of its ties are kept.  Integer sums: any order gives the same. ----
typedef unsigned long long tp_mass_t;  // (the type atomicAdd takes)

// The weight of a float32 word, of a bfloat16 word and of a float16 word (the float32 rule on the
// value widened exactly: sig 2^(E - 25) 2^40 with E <= 14 below 1.0), from the bits alone
__host__ __device__ inline uint64_t tp_weight_f32(uint32_t x) {
    if (x > 0x7F800000u) return 0u;  // the sign bit, or a NaN
    if (x >= 0x3F800000u) return 1ull << TP_FRAC_BITS;
    const uint32_t e = x >> 23, m = x & 0x7FFFFFu;
    const uint64_t sig = e ? (m | 0x800000u) : m;
    const int sh = (int)(e ? e : 1u) - (150 - TP_FRAC_BITS);  // x 2^40 = sig 2^sh, sh <= 16
    if (sh >= 0) return sig << sh;
    return sh > -24 ? sig >> -sh : 0u;
}
__host__ __device__ inline uint64_t tp_weight_f16(uint32_t x) {
    x &= 0xFFFFu;
    if (x > 0x7C00u) return 0u;
    if (x >= 0x3C00u) return 1ull << TP_FRAC_BITS;
    const uint32_t e = x >> 10, m = x & 0x3FFu;
    const uint64_t sig = e ? (m | 0x400u) : m;
    return sig << ((e ? e : 1u) + (uint32_t)(TP_FRAC_BITS - 25));
}
template <int KT>
__device__ __forceinline__ uint64_t tp_w(uint32_t u, uint32_t xr) {
    const uint32_t x = kth_unord<KT>(u, xr);
    if constexpr (KT == KTH_F16) return tp_weight_f16(x);
    else if constexpr (KT == KTH_BF16) return tp_weight_f32(x << 16);
    else return tp_weight_f32(x);
}

// Per row and level, as KthState.  trem == 0: the row's total is zero and the row is kept whole.
struct TpState {
    uint64_t trem;  // what is left of the target among the keys that match the prefix (>= 1)
    uint32_t prefix, d;
};
struct TpArgs {
    const float *d_p;     // [rows], or nullptr: p
    tp_mass_t *hist;      // long rows: [rows][TK_LEVELS][256]
    tp_mass_t *cmass;     // long rows: [rows][nch][256]: each chunk's masses of the current level
    TpState *st;          // long rows: [rows][TK_LEVELS + 1]
    uint32_t *kept_out;   // [rows], or nullptr
    float p;
};

// P of the row's p, from its bits; a p outside (0, 1] is reported in the header by the thread told to
__device__ __forceinline__ uint64_t tp_fixed_p(const TpArgs &tp, uint32_t row, bool report, uint32_t *hdr) {
    const uint32_t b = __float_as_uint(tp.d_p ? tp.d_p[row] : tp.p);
    uint64_t P;
    bool bad = true;
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) P = 1ull << 32;             // NaN
    else if ((b >> 31) || b == 0u) P = 1u;                           // p <= 0
    else if (b > 0x3F800000u) P = 1ull << 32;                        // p > 1
    else {
        bad = false;
        const uint32_t e = b >> 23, m = b & 0x7FFFFFu;
        const uint64_t sig = e ? (m | 0x800000u) : m;
        const int sh = (int)(e ? e : 1u) - 118;  // p 2^32 = sig 2^sh, sh <= 9
        P = sh >= 0 ? sig << sh : sh > -24 ? sig >> -sh : 0u;
        if (P == 0u) P = 1u;
    }
    if (bad && report) hdr[0] = 1u;
    return P;
}
// t of P and W >= 1: the 96-bit product by its two halves
__device__ __forceinline__ uint64_t tp_target(uint64_t P, uint64_t W) {
    const uint64_t hi = __umul64hi(P, W), lo = P * W;
    const uint64_t t = (hi << 32) + (lo >> 32) + ((lo & 0xFFFFFFFFull) ? 1u : 0u);
    return t ? t : 1u;
}

// kth_pick on masses, in two steps, since level 0 needs the total before it has a target.  Called by
// a whole wave on a level histogram of 256 masses (global or LDS); the results are wave-uniform.
struct TpScan {
    uint64_t c[4], run, total;  // digits 4 lane .. 4 lane + 3, the mass below them, the row's
};
__device__ __forceinline__ uint64_t tp_shfl(uint64_t v, int src) { return (uint64_t)__shfl((tp_mass_t)v, src); }
__device__ __forceinline__ TpScan tp_scan(const tp_mass_t *hrow, uint32_t lane) {
    TpScan s;
    uint64_t x = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.c[j] = hrow[4u * lane + (uint32_t)j];
        x += s.c[j];
    }
    const uint64_t own = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((tp_mass_t)x, off);
        if (lane >= (uint32_t)off) x += t;
    }
    s.run = x - own;
    s.total = tp_shfl(x, 63);
    return s;
}
// The d with mass(< d) < trem <= mass(<= d), 1 <= trem <= total
struct TpPick {
    uint32_t d;
    uint64_t below, in;  // the mass below digit d and of digit d
};
__device__ __forceinline__ TpPick tp_find(const TpScan &s, uint64_t trem, uint32_t lane) {
    uint64_t run = s.run, below = 0u, in = 0u;
    uint32_t d = 255u;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!found && run < trem && trem <= run + s.c[j]) {
            found = true;
            d = 4u * lane + (uint32_t)j;
            below = run;
            in = s.c[j];
        }
        run += s.c[j];
    }
    const uint64_t m = __ballot(found);
    const int srcl = m ? __ffsll((long long)m) - 1 : 63;  // (no lane: trem exceeds the total, which cannot happen)
    TpPick p;
    p.d = __shfl(d, srcl);
    p.below = tp_shfl(below, srcl);
    p.in = tp_shfl(in, srcl);
    if (p.below >= trem) p.below = trem - 1u;  // keeps trem >= 1 whatever the histogram held
    return p;
}
// How many of the threshold's ties the rest of the target takes: ceil(trem / w), w = w(T) > 0
__device__ __forceinline__ uint32_t tp_ties_kept(uint64_t trem, uint64_t w) {
    if (w == 0u) w = 1u;  // (cannot happen: the digit picked held mass)
    return (uint32_t)((trem + w - 1u) / w);
}

// Rows of up to BLOCK * KTH_KPT keys: k_kth_short<.., FILTER = true> with the mass select in place
// of the count select, SLOTS replicas of 64-bit words per digit, and the number kept as one block
// sum.  A row without mass is stored as it is and reported in the header.
template <int KT, int BLOCK, int SLOTS>
__global__ __launch_bounds__(BLOCK) void k_tp_short(KthArgs a, TkmArgs m, TpArgs tp) {
    constexpr int E = KTH_E<KT>, T = KTH_KPT / E;
    constexpr int TG = T + 1;  // a row that starts inside a group has one group more
    constexpr int NLEV = kth_levels(KT);
    __shared__ tp_mass_t h[256 * SLOTS];
    __shared__ __attribute__((aligned(16))) tp_mass_t hrow[256];
    __shared__ uint32_t wsum[BLOCK / WAVE], tot, nkept;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const uint32_t mis = group_mis(base, 0u), nq = group_count<E>(0u, a.cols, mis);  // <= T * BLOCK + 1
    uint32_t u[TG][E], vm[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const uint32_t q = (uint32_t)t * BLOCK + tid;
        int64_t i0;
        vm[t] = 0u;
        if (q < nq) vm[t] = kth_load<KT>(base, 0u, a.cols, mis, q, a.xr, u[t], i0);
        else
#pragma unroll
            for (int j = 0; j < E; ++j) u[t][j] = 0u;
    }
    if (tid == 0u) nkept = 0u;  // (the levels' barriers lie between this and the adds)
    const uint64_t P = tp_fixed_p(tp, row, tid == 0u, a.hdr);
    uint32_t prefix = 0u;
    uint64_t trem = 0u, in = 0u;
    bool whole = false;
    for (int level = 0; level < NLEV; ++level) {
        const uint32_t shift = 24u - 8u * (uint32_t)level;
        const uint32_t mask = level ? 0xFFFFFFFFu << (shift + 8u) : 0u;
        for (uint32_t i = tid; i < 256u * SLOTS; i += BLOCK) h[i] = 0u;
        __syncthreads();
        // The weights do not depend on the level: left to itself the compiler computes all of them once
        // and keeps two registers per key (139-172 VGPRs at 256 threads; 128 and 128-224 bytes of scratch
        // per lane at 1024).  An xr that is opaque per level makes every level compute its own.
        uint32_t xr = a.xr;
        asm volatile("" : "+s"(xr));
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int j = 0; j < E; ++j)
                if (((vm[t] >> j) & 1u) && ((u[t][j] ^ prefix) & mask) == 0u) {
                    const uint64_t w = tp_w<KT>(u[t][j], xr);
                    if (w) atomicAdd(&h[((u[t][j] >> shift) & 255u) * SLOTS + (tid & (SLOTS - 1u))], (tp_mass_t)w);
                }
        __syncthreads();
        if (tid < 256u) {
            tp_mass_t sum = 0u;
#pragma unroll
            for (uint32_t q = 0; q < (uint32_t)SLOTS; ++q) sum += h[tid * SLOTS + ((q + tid) & (SLOTS - 1u))];
            hrow[tid] = sum;
        }
        __syncthreads();
        const TpScan sc = tp_scan(hrow, lane);  // (every wave: the same answer)
        if (level == 0) {
            whole = sc.total == 0u;
            if (whole) break;  // (uniform)
            trem = tp_target(P, sc.total);
        }
        const TpPick p = tp_find(sc, trem, lane);
        prefix |= p.d << shift;
        trem -= p.below;
        in = p.in;
    }
    // km[t]: the elements of group (t, tid) that are kept: the keys below the threshold and the first
    // krem of its ties in position order.  All of the ties (uniform): no scan.
    uint32_t km[TG];
    if (whole) {
        if (tid == 0u) a.hdr[0] = 1u;
#pragma unroll
        for (int t = 0; t < TG; ++t) km[t] = vm[t];
    } else {
        const uint64_t wT = tp_w<KT>(prefix, a.xr);
        const uint32_t krem = tp_ties_kept(trem, wT);
        const bool all_ties = LABSORT_TKM_SKIP_SCAN && trem + wT > in;  // in = ties x wT
        uint32_t carry = 0u;
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            uint32_t lt = 0u, em = 0u;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool v = (vm[t] >> j) & 1u;
                lt |= (v && u[t][j] < prefix ? 1u : 0u) << j;
                em |= (v && u[t][j] == prefix ? 1u : 0u) << j;
            }
            km[t] = lt;
            if (all_ties) km[t] |= em;
            else if (carry < krem) {  // (uniform; past it no tie is kept)
                const uint32_t c = (uint32_t)__popc(em);
                const uint32_t before = kth_ordered_step<BLOCK>(c, carry, wsum, &tot);
                const uint32_t room = before < krem ? krem - before : 0u;
                uint32_t seen = 0u;
#pragma unroll
                for (int j = 0; j < E; ++j)
                    if ((em >> j) & 1u) {
                        if (seen < room) km[t] |= 1u << j;
                        ++seen;
                    }
            }
        }
    }
    if (tp.kept_out) {  // (uniform)
        uint32_t mine = 0u;
#pragma unroll
        for (int t = 0; t < TG; ++t) mine += (uint32_t)__popc(km[t]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if (lane == 0u && mine) atomicAdd(&nkept, mine);
        __syncthreads();
        if (tid == 0u) tp.kept_out[row] = nkept;
    }
    if (!m.keys_out && !m.mask_out) return;
    const size_t rowoff = (size_t)row * a.cols;
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const uint32_t q = (uint32_t)t * BLOCK + tid;
        if (q >= nq) continue;
        uint32_t w[E];
#pragma unroll
        for (int j = 0; j < E; ++j) w[j] = (km[t] >> j) & 1u ? kth_unord<KT>(u[t][j], a.xr) : m.fill;
        tkm_store<KT>(m, rowoff, (int64_t)E * q - (int64_t)mis, vm[t], w, km[t]);
    }
}

// Longer rows, per level: one workgroup per (row, chunk) sums the level's digit masses of the keys
// that match the prefix, per chunk (cmass, plain stores) and per row (hist, one atomic add per
// digit that holds mass).  From level 1 on a chunk is read only if it held mass of the digit chosen
// before; a skipped chunk's row of cmass is zeroed, as k_kth_hist zeroes its counts.
template <int KT>
__global__ __launch_bounds__(KTH_BLOCK) void k_tp_hist(KthArgs a, TpArgs tp, int level) {
    constexpr int E = KTH_E<KT>, T = KTH_KPT / E;
    __shared__ tp_mass_t h[256 * TP_SLOTS];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / a.nch, c = blockIdx.x - row * a.nch;
    TpState st{0u, 0u, 0u};
    if (level) st = tp.st[(size_t)row * (TK_LEVELS + 1) + level];
    tp_mass_t *crow = tp.cmass + ((size_t)row * a.nch + c) * 256u;
    // every thread reads the same word, which only this workgroup writes, and only zero over zero
    // before the barriers below
    if (level && __builtin_amdgcn_readfirstlane((uint32_t)(st.trem != 0u && crow[st.d] != 0u)) == 0u) {
        if (tid < 256u) crow[tid] = 0u;  // (no stale masses of the level before)
        return;
    }
    const uint32_t shift = 24u - 8u * (uint32_t)level;
    const uint32_t mask = level ? 0xFFFFFFFFu << (shift + 8u) : 0u;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const uint32_t xr = a.xr, prefix = st.prefix;
    for (uint32_t i = tid; i < 256u * TP_SLOTS; i += KTH_BLOCK) h[i] = 0u;
    __syncthreads();
    const KthChunk ch = kth_chunk<KT>(base, a.cols, c);
    for (uint32_t q0 = 0; q0 < ch.nq; q0 += (uint32_t)T * KTH_BLOCK) {
        uint32_t u[T][E], vm[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t q = q0 + (uint32_t)t * KTH_BLOCK + tid;
            int64_t i0;
            vm[t] = 0u;
            if (q < ch.nq) vm[t] = kth_load<KT>(base, ch.beg, ch.end, ch.mis, q, xr, u[t], i0);
            else
#pragma unroll
                for (int j = 0; j < E; ++j) u[t][j] = 0u;
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int j = 0; j < E; ++j)
                if (((vm[t] >> j) & 1u) && ((u[t][j] ^ prefix) & mask) == 0u) {
                    const uint64_t w = tp_w<KT>(u[t][j], xr);
                    if (w) atomicAdd(&h[((u[t][j] >> shift) & 255u) * TP_SLOTS + (tid & (TP_SLOTS - 1u))], (tp_mass_t)w);
                }
    }
    __syncthreads();
    if (tid < 256u) {
        tp_mass_t sum = 0u;
#pragma unroll 8
        for (uint32_t q = 0; q < (uint32_t)TP_SLOTS; ++q) sum += h[tid * TP_SLOTS + ((q + tid) & (TP_SLOTS - 1u))];
        crow[tid] = sum;
        if (sum) atomicAdd(&tp.hist[((size_t)row * TK_LEVELS + level) * 256u + tid], sum);
    }
}

// One workgroup per row: the digit at which the running mass reaches what is left of the target,
// and the next level's state.  Level 0 reads the row's p and clears its kept count.  After the
// last level it divides each chunk's mass of the last digit by w(T), which is the chunk's count of
// T, finds the chunk that holds the last tie kept and writes the KthState that k_kth_locate and
// k_tkm_apply read.  A row without mass gets the pair that keeps everything.
template <int KT>
__global__ __launch_bounds__(KTH_BLOCK) void k_tp_pick(KthArgs a, TpArgs tp, int level) {
    constexpr int NLEV = kth_levels(KT);
    __shared__ uint32_t wsum[KTH_BLOCK / WAVE], tot, hit[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, row = blockIdx.x;
    TpState st{0u, 0u, 0u};
    if (level) st = tp.st[(size_t)row * (TK_LEVELS + 1) + level];
    const TpScan sc = tp_scan(tp.hist + ((size_t)row * TK_LEVELS + level) * 256u, lane);
    if (level == 0) {
        if (tid == 0u && tp.kept_out) tp.kept_out[row] = 0u;
        const uint64_t P = tp_fixed_p(tp, row, tid == 0u, a.hdr);
        if (sc.total) st.trem = tp_target(P, sc.total);
        else if (tid == 0u) a.hdr[0] = 1u;
    }
    const bool last = level == NLEV - 1;
    TpState *out = tp.st + (size_t)row * (TK_LEVELS + 1) + level + 1;
    KthState *kout = a.st + (size_t)row * (TK_LEVELS + 1) + NLEV;
    if (st.trem == 0u) {  // (uniform) krem == 0: k_kth_locate leaves the position alone
        if (tid == 0u) {
            if (!last) *out = TpState{0u, 0u, 0u};
            else {
                *kout = KthState{0xFFFFFFFFu, 0u, 0u, 0u};
                a.idx_out[row] = a.cols - 1u;
            }
        }
        return;
    }
    const TpPick p = tp_find(sc, st.trem, lane);
    TpState ns;
    ns.prefix = st.prefix | (p.d << (24u - 8u * (uint32_t)level));
    ns.trem = st.trem - p.below;
    ns.d = p.d;
    if (!last) {
        if (tid == 0u) *out = ns;
        return;
    }
    uint64_t wT = tp_w<KT>(ns.prefix, a.xr);
    if (wT == 0u) wT = 1u;  // (cannot happen: the digit picked held mass)
    const uint32_t krem = tp_ties_kept(ns.trem, wT);
    if (tid == 0u) {
        hit[0] = 0u;
        hit[1] = 1u;
    }
    __syncthreads();
    uint32_t carry = 0u;
    for (uint32_t b = 0; b < a.nch && carry < krem; b += KTH_BLOCK) {  // (uniform)
        const uint32_t c = b + tid;
        const uint32_t v = c < a.nch ? (uint32_t)(tp.cmass[((size_t)row * a.nch + c) * 256u + p.d] / wT) : 0u;
        const uint32_t before = kth_ordered_step(v, carry, wsum, &tot);
        if (v && before < krem && krem <= before + v) {
            hit[0] = c;
            hit[1] = krem - before;
        }
    }
    __syncthreads();
    if (tid == 0u) *kout = KthState{ns.prefix, hit[1], p.d, hit[0]};
}

// ---- categorical sampling (labsort_sample_device): positions drawn by exact inverse CDF.  With the
// weights above, W the row's total and U a caller's uniform 32-bit word, the target is
// s = floor(U W / 2^32) < W and the draw is the smallest position whose inclusive prefix of weights,
// in position order, exceeds s.  A prefix sum and a search: no sort, no select, no histogram.
// Integer sums: any order gives the same. ----
constexpr uint32_t SMP_NO_DRAW = 0xFFFFFFFFu;  // the position a row without mass draws, and its chunk
struct SmpDraw {
    uint64_t s;      // what is left of the draw's target inside its chunk
    uint32_t chunk;  // SMP_NO_DRAW: the row has no mass
    uint32_t pad;
};
static_assert(sizeof(SmpDraw) == 16, "labsort.h states the size of a draw state");
struct SmpArgs {
    const uint32_t *u;  // [rows][ndraw]
    uint32_t *idx_out;  // [rows][ndraw]
    uint64_t *cmass;    // long rows: [rows][nch]
    SmpDraw *draw;      // long rows: [rows][ndraw]
    uint32_t ndraw;
    uint32_t first;     // k_smp_short, k_smp_locate: the launch's first workgroup, of rows or rows x ndraw
};

// s of U and W < 2^63: the 95-bit product by its two halves (tp_target's, rounded down)
__device__ __forceinline__ uint64_t smp_target(uint32_t U, uint64_t W) {
    const uint64_t hi = __umul64hi((uint64_t)U, W), lo = (uint64_t)U * W;
    return (hi << 32) | (lo >> 32);
}
// Inclusive prefix sum of x over the wave's lanes (all 64 active): wave_incl_scan on 64-bit words
__device__ __forceinline__ uint64_t smp_wave_scan(uint64_t x, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t t = tp_shfl(x, (int)lane - off);
        if (lane >= (uint32_t)off) x += t;
    }
    return x;
}

// Up to BLOCK * KTH_KPT keys [beg, end) of a row in the registers of one workgroup, as k_tp_short holds
// them: thread tid has groups q = t BLOCK + tid, and of each the mass c and the mass lo of
// everything before it in position order.
template <int KT, int BLOCK>
struct SmpRow {
    static constexpr int E = KTH_E<KT>, TG = KTH_KPT / E + 1, NW = BLOCK / WAVE, NE = TG * NW;
    uint32_t u[TG][E], vm[TG];
    uint64_t lo[TG], c[TG];
};
// Loads and scans; returns the total.  The 64-bit twin of kth_ordered_step, for all stripes at once:
// a wave scan per stripe, the wave totals in LDS in position order (stripe, wave), one barrier, and
// every wave scans those NE totals for what lies before each of its stripes.
template <int KT, int BLOCK>
__device__ __forceinline__ uint64_t smp_scan(SmpRow<KT, BLOCK> &r, const kth_elem_t<KT> *base, uint32_t beg, uint32_t end,
                                             uint32_t mis, uint32_t nq, uint32_t xr, uint64_t *wtot) {
    using R = SmpRow<KT, BLOCK>;
    constexpr int E = R::E, TG = R::TG, NW = R::NW, NE = R::NE, H = (NE + 63) / 64;
    static_assert(64 % NW == 0, "a stripe's wave totals lie in one 64-entry half");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const uint32_t q = (uint32_t)t * BLOCK + tid;
        int64_t i0;
        r.vm[t] = 0u;
        if (q < nq) r.vm[t] = kth_load<KT>(base, beg, end, mis, q, xr, r.u[t], i0);
        else
#pragma unroll
            for (int j = 0; j < E; ++j) r.u[t][j] = 0u;
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        uint64_t c = 0u;
#pragma unroll
        for (int j = 0; j < E; ++j)
            if ((r.vm[t] >> j) & 1u) c += tp_w<KT>(r.u[t][j], xr);
        const uint64_t inc = smp_wave_scan(c, lane);
        r.c[t] = c;
        r.lo[t] = inc - c;
        if (lane == 63u) wtot[(uint32_t)t * NW + wid] = inc;
    }
    __syncthreads();
    uint64_t ex[H], total = 0u;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const uint32_t e = 64u * (uint32_t)h + lane;
        const uint64_t v = e < (uint32_t)NE ? wtot[e] : 0u;
        const uint64_t inc = smp_wave_scan(v, lane);
        ex[h] = total + inc - v;
        total += tp_shfl(inc, 63);
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) r.lo[t] += tp_shfl(ex[(t * NW) / 64], (int)(((uint32_t)t * NW + wid) & 63u));
    return total;
}
// The draw of target s < total: the one thread whose group has lo <= s < lo + c walks its elements
// and stores the position.  No barrier.
template <int KT, int BLOCK>
__device__ __forceinline__ void smp_find(const SmpRow<KT, BLOCK> &r, uint64_t s, uint32_t xr, uint32_t beg, uint32_t mis,
                                         uint32_t *out) {
    using R = SmpRow<KT, BLOCK>;
    constexpr int E = R::E, TG = R::TG;
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        if (s - r.lo[t] >= r.c[t]) continue;  // (s < lo wraps to more than any c)
        uint64_t run = r.lo[t];
        uint32_t at = 0u;
        bool found = false;
#pragma unroll
        for (int j = 0; j < E; ++j)
            if ((r.vm[t] >> j) & 1u) {
                run += tp_w<KT>(r.u[t][j], xr);
                if (!found && s < run) {
                    found = true;
                    at = (uint32_t)j;
                }
            }
        *out = beg - mis + (uint32_t)E * ((uint32_t)t * BLOCK + threadIdx.x) + at;  // (at >= mis in the row's first group)
    }
}

// Rows of up to BLOCK * KTH_KPT keys: one launch, one workgroup per row, every draw of the row from
// the row in registers.  A row without mass stores SMP_NO_DRAW and reports in the header.
template <int KT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_smp_short(KthArgs a, SmpArgs sm) {
    using R = SmpRow<KT, BLOCK>;
    __shared__ uint64_t wtot[R::NE];
    const uint32_t tid = threadIdx.x, row = sm.first + blockIdx.x;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const uint32_t mis = group_mis(base, 0u), nq = group_count<R::E>(0u, a.cols, mis);  // <= T * BLOCK + 1
    R r;
    const uint64_t W = smp_scan<KT, BLOCK>(r, base, 0u, a.cols, mis, nq, a.xr, wtot);
    const uint32_t *urow = sm.u + (size_t)row * sm.ndraw;
    uint32_t *orow = sm.idx_out + (size_t)row * sm.ndraw;
    if (W == 0u) {  // (uniform)
        if (tid == 0u) a.hdr[0] = 1u;
        for (uint32_t d = tid; d < sm.ndraw; d += BLOCK) orow[d] = SMP_NO_DRAW;
        return;
    }
    for (uint32_t d = 0; d < sm.ndraw; ++d) {
        // The weights do not depend on the draw: left to itself the compiler computes all of them ahead
        // of the loop and keeps two registers per key (136 VGPRs at 256 threads, 44 bytes of scratch per
        // lane at 1024 for bfloat16).  An xr that is opaque per draw makes the one walk compute its own.
        uint32_t xr = a.xr;
        asm volatile("" : "+s"(xr));
        smp_find<KT, BLOCK>(r, smp_target(urow[d], W), xr, 0u, mis, orow + d);
    }
}

// Longer rows.  One workgroup per (row, chunk): the chunk's mass, a plain store.
template <int KT>
__global__ __launch_bounds__(KTH_BLOCK) void k_smp_sum(KthArgs a, SmpArgs sm) {
    constexpr int E = KTH_E<KT>, T = KTH_KPT / E, NW = KTH_BLOCK / WAVE;
    __shared__ uint64_t wtot[NW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t row = blockIdx.x / a.nch, c = blockIdx.x - row * a.nch;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const uint32_t xr = a.xr;
    const KthChunk ch = kth_chunk<KT>(base, a.cols, c);
    uint64_t mine = 0u;
    for (uint32_t q0 = 0; q0 < ch.nq; q0 += (uint32_t)T * KTH_BLOCK) {
        uint32_t u[T][E], vm[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t q = q0 + (uint32_t)t * KTH_BLOCK + tid;
            int64_t i0;
            vm[t] = 0u;
            if (q < ch.nq) vm[t] = kth_load<KT>(base, ch.beg, ch.end, ch.mis, q, xr, u[t], i0);
            else
#pragma unroll
                for (int j = 0; j < E; ++j) u[t][j] = 0u;
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int j = 0; j < E; ++j)
                if ((vm[t] >> j) & 1u) mine += tp_w<KT>(u[t][j], xr);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += tp_shfl(mine, (int)(lane ^ (uint32_t)off));
    if (lane == 0u) wtot[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0u) {
        uint64_t sum = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += wtot[w];
        sm.cmass[(size_t)row * a.nch + c] = sum;
    }
}

// One workgroup per row: the running sums of the row's chunk masses (thread tid: chunk tid), and per
// draw the chunk whose range of the prefix holds the target, with what is left of the target inside
// it.  A row without mass stores SMP_NO_DRAW to its draws and their states and reports in the header.
__global__ __launch_bounds__(SMP_MAX_CHUNKS) void k_smp_pick(KthArgs a, SmpArgs sm) {
    constexpr int NW = SMP_MAX_CHUNKS / WAVE;
    __shared__ uint64_t wtot[NW], cum[SMP_MAX_CHUNKS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6, row = blockIdx.x;
    const uint32_t nch = a.nch < (uint32_t)SMP_MAX_CHUNKS ? a.nch : (uint32_t)SMP_MAX_CHUNKS;
    const uint64_t v = tid < nch ? sm.cmass[(size_t)row * a.nch + tid] : 0u;
    uint64_t inc = smp_wave_scan(v, lane);
    if (lane == 63u) wtot[wid] = inc;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if ((uint32_t)w < wid) inc += wtot[w];
    cum[tid] = inc;
    __syncthreads();
    const uint64_t W = cum[SMP_MAX_CHUNKS - 1];
    const uint32_t *urow = sm.u + (size_t)row * sm.ndraw;
    uint32_t *orow = sm.idx_out + (size_t)row * sm.ndraw;
    SmpDraw *drow = sm.draw + (size_t)row * sm.ndraw;
    if (W == 0u && tid == 0u) a.hdr[0] = 1u;
    for (uint32_t d = tid; d < sm.ndraw; d += SMP_MAX_CHUNKS) {
        if (W == 0u) {
            orow[d] = SMP_NO_DRAW;
            drow[d] = SmpDraw{0u, SMP_NO_DRAW, 0u};
            continue;
        }
        const uint64_t s = smp_target(urow[d], W);
        uint32_t lo = 0u, hi = nch - 1u;  // the first chunk with cum > s: cum[nch - 1] = W > s
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cum[mid] > s) hi = mid;
            else lo = mid + 1u;
        }
        drow[d] = SmpDraw{s - (lo ? cum[lo - 1u] : 0u), lo, 0u};
    }
}

// One workgroup per (row, draw): the draw's chunk in registers and k_smp_short's search on what is
// left of the target.
template <int KT>
__global__ __launch_bounds__(KTH_BLOCK) void k_smp_locate(KthArgs a, SmpArgs sm) {
    using R = SmpRow<KT, KTH_BLOCK>;
    __shared__ uint64_t wtot[R::NE];
    const uint32_t at = sm.first + blockIdx.x;  // the draw, of rows x ndraw
    const uint32_t row = at / sm.ndraw;
    const SmpDraw dr = sm.draw[at];
    if (dr.chunk == SMP_NO_DRAW) return;  // (uniform: k_smp_pick stored the draw)
    const uint32_t c = dr.chunk < a.nch ? dr.chunk : a.nch - 1u;
    const kth_elem_t<KT> *base = kth_row<KT>(a, row);
    const KthChunk ch = kth_chunk<KT>(base, a.cols, c);
    R r;
    smp_scan<KT, KTH_BLOCK>(r, base, ch.beg, ch.end, ch.mis, ch.nq, a.xr, wtot);
    smp_find<KT, KTH_BLOCK>(r, dr.s, a.xr, ch.beg, ch.mis, sm.idx_out + at);
}

// ---- launches.  kt: KthKey, the instantiation that runs: f gets it as a constant ----
template <class F>
void kth_dispatch(int kt, F f) {
    if (kt == KTH_BF16) f(std::integral_constant<int, KTH_BF16>{});
    else if (kt == KTH_F16) f(std::integral_constant<int, KTH_F16>{});
    else if (kt == KTH_F32) f(std::integral_constant<int, KTH_F32>{});
    else f(std::integral_constant<int, KTH_INT>{});
}

// FILTER = false: the select (m: TkmArgs{}).  FILTER = true: the top-k filter.
template <bool FILTER>
hipError_t launch_kth_short(const KthArgs &a, const TkmArgs &m, size_t rows, int kt, hipStream_t s) {
    const unsigned grid = (unsigned)rows;
    kth_dispatch(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        if (a.cols <= (uint32_t)KTH_SMALL_ROW_KEYS)
            k_kth_short<KT, KTH_SMALL_BLOCK, KTH_SMALL_SLOTS, FILTER><<<grid, KTH_SMALL_BLOCK, 0, s>>>(a, m);
        else k_kth_short<KT, KTH_BLOCK, TK_SLOTS, FILTER><<<grid, KTH_BLOCK, 0, s>>>(a, m);
    });
    return hipGetLastError();
}

hipError_t launch_kth_hist(const KthArgs &a, size_t rows, int level, int kt, hipStream_t s) {
    const uint32_t g = (a.nch + TK_MAX_HIST_WG - 1u) / TK_MAX_HIST_WG;  // chunks per workgroup
    const uint32_t nx = (a.nch + g - 1u) / g;
    const unsigned grid = (unsigned)(rows * nx);
    kth_dispatch(kt, [&](auto K) { k_kth_hist<decltype(K)::value><<<grid, KTH_BLOCK, 0, s>>>(a, level, nx, g); });
    return hipGetLastError();
}

hipError_t launch_kth_pick(const KthArgs &a, size_t rows, int level, int kt, hipStream_t s) {
    k_kth_pick<<<(unsigned)rows, KTH_BLOCK, 0, s>>>(a, level, level == kth_levels(kt) - 1, kt);
    return hipGetLastError();
}

hipError_t launch_kth_locate(const KthArgs &a, size_t rows, int kt, hipStream_t s) {
    kth_dispatch(kt, [&](auto K) { k_kth_locate<decltype(K)::value><<<(unsigned)rows, KTH_BLOCK, 0, s>>>(a); });
    return hipGetLastError();
}

// kept: nullptr, or (top-p filtering) one zeroed word per row that receives the number of elements kept
hipError_t launch_tkm_apply(const KthArgs &a, const TkmArgs &m, uint32_t *kept, size_t rows, int kt, hipStream_t s) {
    const unsigned grid = (unsigned)(rows * a.nch);
    kth_dispatch(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        if (kept) k_tkm_apply<KT, true><<<grid, KTH_BLOCK, 0, s>>>(a, m, kept);
        else k_tkm_apply<KT, false><<<grid, KTH_BLOCK, 0, s>>>(a, m, nullptr);
    });
    return hipGetLastError();
}

// Longer rows: a histogram and a pick per level, then the position where the call has one
int run_kth_long(const KthArgs &a, size_t rows, int kt, hipStream_t s) {
    for (int level = 0; level < kth_levels(kt); ++level) {
        HIP_TRY(launch_kth_hist(a, rows, level, kt, s));
        HIP_TRY(launch_kth_pick(a, rows, level, kt, s));
    }
    if (a.idx_out) HIP_TRY(launch_kth_locate(a, rows, kt, s));
    return LABSORT_OK;
}

// header | hist | per-row states | per-chunk counts.  Header and histograms are the only words a
// call relies on being clear.  A short row needs the header alone.
struct KthLayout {
    size_t nch, off_hist, zero_bytes, off_st, off_cnt, total;
};
KthLayout kth_layout(size_t rows, size_t cols) {
    KthLayout L{};
    Carver c;
    c.take(KTH_HDR_BYTES);
    L.zero_bytes = L.total = c.o;
    if (rows == 0 || cols <= (size_t)KTH_ROW_KEYS) return L;
    L.nch = (cols + TK_CHUNK - 1) / TK_CHUNK;
    L.off_hist = c.take(rows * TK_LEVELS * 256 * sizeof(uint32_t));
    L.zero_bytes = c.o;
    L.off_st = c.take(rows * (TK_LEVELS + 1) * sizeof(KthState));
    L.off_cnt = c.take(rows * L.nch * 256 * sizeof(uint32_t));
    L.total = c.o;
    return L;
}

// The filter's workspace: kth's, then for long rows the words its select writes per row: the
// position of the k-th pair and the key (which the apply pass reads as u from the states instead).
struct TkmLayout {
    KthLayout kth;
    size_t off_pos, off_key, total;
};
TkmLayout tkm_layout(size_t rows, size_t cols) {
    TkmLayout L{};
    L.kth = kth_layout(rows, cols);
    L.total = L.kth.total;
    if (!L.kth.nch) return L;
    Carver c;
    c.o = L.kth.total;
    L.off_pos = c.take(rows * sizeof(uint32_t));
    L.off_key = c.take(rows * sizeof(uint32_t));
    L.total = c.o;
    return L;
}

// What both entry points refuse alike, rows and cols != 0: the key type, a host k outside
// [1, cols], more than 2^31 - 1 elements, a 16-bit key pointer at an odd address (keys_out may be
// nullptr).  Outputs and aliases are each entry's own.
bool kth_call_ok(const void *d_keys, const void *d_keys_out, size_t rows, size_t cols, size_t k, const uint32_t *d_k, int key_type) {
    if (!d_keys || !topk_key_type_ok(key_type)) return false;
    if (!d_k && (k == 0 || k > cols)) return false;
    if (rows > (size_t)0x7FFFFFFFu / cols) return false;
    return !(key_type_is16(key_type) && (((uintptr_t)d_keys | (uintptr_t)d_keys_out) & 1u));
}

// A checked call's key type as KthKey and what its kernels read, but for the outputs: the input,
// k, the order and, for long rows (L.nch != 0), the workspace's tables
struct KthCall {
    int kt;
    KthArgs a;
};
KthCall kth_call(const void *d_keys, size_t cols, size_t k, const uint32_t *d_k, int largest, int key_type, void *d_ws, const KthLayout &L) {
    char *ws = static_cast<char *>(d_ws);
    KthCall c{};
    c.kt = key_type == LABSORT_KEY_F32 ? KTH_F32 : key_type == LABSORT_KEY_BF16 ? KTH_BF16 : key_type == LABSORT_KEY_F16 ? KTH_F16 : KTH_INT;
    c.a.keys = d_keys;
    c.a.d_k = d_k;
    c.a.hdr = reinterpret_cast<uint32_t *>(ws);
    c.a.cols = (uint32_t)cols;
    c.a.k = (uint32_t)(d_k ? 1 : k);
    c.a.nch = (uint32_t)L.nch;
    // 16-bit keys: u = (ord16(key) << 16) ^ xr, its low half clear
    c.a.xr = kth_is16(c.kt) ? (largest ? 0xFFFF0000u : 0u) : flip_of(key_type) ^ (largest ? 0xFFFFFFFFu : 0u);
    if (L.nch) {
        c.a.hist = reinterpret_cast<uint32_t *>(ws + L.off_hist);
        c.a.st = reinterpret_cast<KthState *>(ws + L.off_st);
        c.a.cnt = reinterpret_cast<uint32_t *>(ws + L.off_cnt);
    }
    return c;
}

// ---- top-p filtering: launches and workspace.  Only the float key types reach these ----
template <class F>
void tp_dispatch(int kt, F f) {
    if (kt == KTH_BF16) f(std::integral_constant<int, KTH_BF16>{});
    else if (kt == KTH_F16) f(std::integral_constant<int, KTH_F16>{});
    else f(std::integral_constant<int, KTH_F32>{});
}

hipError_t launch_tp_short(const KthArgs &a, const TkmArgs &m, const TpArgs &tp, size_t rows, int kt, hipStream_t s) {
    const unsigned grid = (unsigned)rows;
    tp_dispatch(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        if (a.cols <= (uint32_t)KTH_SMALL_ROW_KEYS)
            k_tp_short<KT, KTH_SMALL_BLOCK, TP_SMALL_SLOTS><<<grid, KTH_SMALL_BLOCK, 0, s>>>(a, m, tp);
        else k_tp_short<KT, KTH_BLOCK, TP_SLOTS><<<grid, KTH_BLOCK, 0, s>>>(a, m, tp);
    });
    return hipGetLastError();
}

// Longer rows: a mass histogram and a pick per level, the position of the last pair kept, the
// streaming pass (which counts what it keeps where the call asks for the count)
int run_tp_long(const KthArgs &a, const TkmArgs &m, const TpArgs &tp, size_t rows, int kt, hipStream_t s) {
    const unsigned grid = (unsigned)(rows * a.nch);
    for (int level = 0; level < kth_levels(kt); ++level) {
        tp_dispatch(kt, [&](auto K) { k_tp_hist<decltype(K)::value><<<grid, KTH_BLOCK, 0, s>>>(a, tp, level); });
        HIP_TRY(hipGetLastError());
        tp_dispatch(kt, [&](auto K) { k_tp_pick<decltype(K)::value><<<(unsigned)rows, KTH_BLOCK, 0, s>>>(a, tp, level); });
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(launch_kth_locate(a, rows, kt, s));
    HIP_TRY(launch_tkm_apply(a, m, tp.kept_out, rows, kt, s));
    return LABSORT_OK;
}

// header | mass histograms | the mass select's states | the final KthState slots | per-chunk masses |
// the position and the key of each row's last pair kept.  Header and histograms are the only words
// a call relies on being clear.  A short row needs the header alone.
struct TpLayout {
    size_t nch, off_hist, zero_bytes, off_tst, off_st, off_cmass, off_pos, off_key, total;
};
TpLayout tp_layout(size_t rows, size_t cols) {
    TpLayout L{};
    Carver c;
    c.take(KTH_HDR_BYTES);
    L.zero_bytes = L.total = c.o;
    if (rows == 0 || cols <= (size_t)KTH_ROW_KEYS) return L;
    L.nch = (cols + TK_CHUNK - 1) / TK_CHUNK;
    L.off_hist = c.take(rows * TK_LEVELS * 256 * sizeof(tp_mass_t));
    L.zero_bytes = c.o;
    L.off_tst = c.take(rows * (TK_LEVELS + 1) * sizeof(TpState));
    L.off_st = c.take(rows * (TK_LEVELS + 1) * sizeof(KthState));
    L.off_cmass = c.take(rows * L.nch * 256 * sizeof(tp_mass_t));
    L.off_pos = c.take(rows * sizeof(uint32_t));
    L.off_key = c.take(rows * sizeof(uint32_t));
    L.total = c.o;
    return L;
}

// ---- categorical sampling: launches and workspace ----
// A grid of up to 2^31 - 1 workgroups (rows, or rows x ndraw) goes out in launches of at most
// SMP_MAX_GRID: the runtime takes no grid of 2^32 threads or more.  f(sm, grid) launches the
// workgroups sm.first .. sm.first + grid - 1.  One launch for everything but the largest calls.
template <class F>
hipError_t smp_launches(SmpArgs sm, size_t total, F f) {
    for (size_t first = 0; first < total; first += SMP_MAX_GRID) {
        sm.first = (uint32_t)first;
        f(sm, (unsigned)(total - first < (size_t)SMP_MAX_GRID ? total - first : (size_t)SMP_MAX_GRID));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_smp_short(const KthArgs &a, const SmpArgs &sm, size_t rows, int kt, hipStream_t s) {
    return smp_launches(sm, rows, [&](const SmpArgs &part, unsigned grid) {
        tp_dispatch(kt, [&](auto K) {
            constexpr int KT = decltype(K)::value;
            if (a.cols <= (uint32_t)KTH_SMALL_ROW_KEYS) k_smp_short<KT, KTH_SMALL_BLOCK><<<grid, KTH_SMALL_BLOCK, 0, s>>>(a, part);
            else k_smp_short<KT, KTH_BLOCK><<<grid, KTH_BLOCK, 0, s>>>(a, part);
        });
    });
}

// Longer rows: the chunk masses, each draw's chunk, each draw's position.  rows x chunks and rows
// are far below SMP_MAX_GRID here (rows x cols <= 2^31 - 1 with cols > KTH_ROW_KEYS).
int run_smp_long(const KthArgs &a, const SmpArgs &sm, size_t rows, int kt, hipStream_t s) {
    tp_dispatch(kt, [&](auto K) { k_smp_sum<decltype(K)::value><<<(unsigned)(rows * a.nch), KTH_BLOCK, 0, s>>>(a, sm); });
    HIP_TRY(hipGetLastError());
    k_smp_pick<<<(unsigned)rows, SMP_MAX_CHUNKS, 0, s>>>(a, sm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(smp_launches(sm, rows * sm.ndraw, [&](const SmpArgs &part, unsigned grid) {
        tp_dispatch(kt, [&](auto K) { k_smp_locate<decltype(K)::value><<<grid, KTH_BLOCK, 0, s>>>(a, part); });
    }));
    return LABSORT_OK;
}

// header | per-chunk masses | per-draw states.  The header is the only word a call relies on being
// clear.  A short row needs the header alone.
struct SmpLayout {
    size_t nch, off_cmass, off_draw, total;
};
SmpLayout smp_layout(size_t rows, size_t cols, size_t ndraw) {
    SmpLayout L{};
    Carver c;
    c.take(KTH_HDR_BYTES);
    L.total = c.o;
    if (rows == 0 || ndraw == 0 || cols <= (size_t)KTH_ROW_KEYS) return L;
    L.nch = (cols + TK_CHUNK - 1) / TK_CHUNK;
    L.off_cmass = c.take(rows * L.nch * sizeof(uint64_t));
    L.off_draw = c.take(rows * ndraw * sizeof(SmpDraw));
    L.total = c.o;
    return L;
}

}  // namespace

}  // namespace labsort

using namespace labsort;

extern "C" {

size_t labsort_kth_row_keys(void) { return (size_t)KTH_ROW_KEYS; }

size_t labsort_kth_workspace_bytes(size_t rows, size_t cols) { return kth_layout(rows, cols).total; }

int labsort_kth_device(const void *d_keys, size_t rows, size_t cols, size_t k, const uint32_t *d_k, int largest, int key_type,
                       void *d_keys_out, uint32_t *d_idx_out, void *d_ws, size_t ws_bytes, void *stream) {
    static_assert(KTH_HDR_BYTES == 256, "labsort.h states the header's size");
    if (rows == 0 || cols == 0) return LABSORT_OK;
    if (!d_keys_out || !kth_call_ok(d_keys, d_keys_out, rows, cols, k, d_k, key_type)) return LABSORT_ERR_ARG;
    const size_t esz = key_type_is16(key_type) ? 2 : 4;  // bytes per key
    if (d_idx_out == d_keys_out) return LABSORT_ERR_ARG;
    const size_t in_bytes = rows * cols * esz, ko_bytes = rows * esz, w_bytes = rows * 4;
    if (ranges_overlap(d_keys, in_bytes, d_keys_out, ko_bytes)) return LABSORT_ERR_ARG;
    if (d_idx_out && (ranges_overlap(d_keys, in_bytes, d_idx_out, w_bytes) || ranges_overlap(d_keys_out, ko_bytes, d_idx_out, w_bytes)))
        return LABSORT_ERR_ARG;
    if (d_k && ranges_overlap(d_k, w_bytes, d_keys_out, ko_bytes)) return LABSORT_ERR_ARG;
    if (d_k && d_idx_out && ranges_overlap(d_k, w_bytes, d_idx_out, w_bytes)) return LABSORT_ERR_ARG;
    const KthLayout L = kth_layout(rows, cols);
    if (!d_ws || ws_bytes < L.total) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    KthCall c = kth_call(d_keys, cols, k, d_k, largest, key_type, d_ws, L);
    c.a.keys_out = d_keys_out;
    c.a.idx_out = d_idx_out;
    HIP_TRY(launch_zero(d_ws, L.zero_bytes, s));  // (a kernel: graph-replayable)
    TimingScope ts(LABSORT_K_TOPK, s);
    if (cols > (size_t)KTH_ROW_KEYS) return run_kth_long(c.a, rows, c.kt, s);
    HIP_TRY(launch_kth_short<false>(c.a, TkmArgs{}, rows, c.kt, s));
    return LABSORT_OK;
}

int labsort_kth_workspace_status(const void *d_ws, void *stream) {
    uint32_t w = 0;
    if (const int st = read_ws_words(d_ws, &w, 1, as_stream(stream))) return st;
    return w ? LABSORT_ERR_ARG : LABSORT_OK;
}

size_t labsort_topk_mask_workspace_bytes(size_t rows, size_t cols) { return tkm_layout(rows, cols).total; }

int labsort_topk_mask_device(const void *d_keys, size_t rows, size_t cols, size_t k, const uint32_t *d_k, int largest,
                             int key_type, uint32_t fill_bits, void *d_keys_out, uint8_t *d_mask_out, void *d_ws,
                             size_t ws_bytes, void *stream) {
    if (rows == 0 || cols == 0) return LABSORT_OK;
    if (!d_keys_out && !d_mask_out) return LABSORT_ERR_ARG;
    if (!kth_call_ok(d_keys, d_keys_out, rows, cols, k, d_k, key_type)) return LABSORT_ERR_ARG;
    const bool k16 = key_type_is16(key_type);
    const size_t esz = k16 ? 2 : 4;  // bytes per key
    if (k16 && (fill_bits >> 16)) return LABSORT_ERR_ARG;
    // the one alias: the keys written over the input, element for element
    const size_t key_bytes = rows * cols * esz, mask_bytes = rows * cols, w_bytes = rows * 4;
    if (d_keys_out && d_keys_out != d_keys && ranges_overlap(d_keys, key_bytes, d_keys_out, key_bytes)) return LABSORT_ERR_ARG;
    if (d_mask_out && ranges_overlap(d_keys, key_bytes, d_mask_out, mask_bytes)) return LABSORT_ERR_ARG;
    if (d_mask_out && d_keys_out && ranges_overlap(d_keys_out, key_bytes, d_mask_out, mask_bytes)) return LABSORT_ERR_ARG;
    if (d_k && ranges_overlap(d_k, w_bytes, d_keys, key_bytes)) return LABSORT_ERR_ARG;
    if (d_k && d_keys_out && ranges_overlap(d_k, w_bytes, d_keys_out, key_bytes)) return LABSORT_ERR_ARG;
    if (d_k && d_mask_out && ranges_overlap(d_k, w_bytes, d_mask_out, mask_bytes)) return LABSORT_ERR_ARG;
    const TkmLayout L = tkm_layout(rows, cols);
    if (!d_ws || ws_bytes < L.total) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    KthCall c = kth_call(d_keys, cols, k, d_k, largest, key_type, d_ws, L.kth);
    TkmArgs m{};
    m.keys_out = d_keys_out;
    m.mask_out = d_mask_out;
    m.fill = fill_bits;
    HIP_TRY(launch_zero(ws, L.kth.zero_bytes, s));
    TimingScope ts(LABSORT_K_TOPK, s);
    if (cols <= (size_t)KTH_ROW_KEYS) {
        HIP_TRY(launch_kth_short<true>(c.a, m, rows, c.kt, s));
        return LABSORT_OK;
    }
    // the select with positions, its outputs in the workspace, then the streaming pass
    c.a.keys_out = ws + L.off_key;
    c.a.idx_out = reinterpret_cast<uint32_t *>(ws + L.off_pos);
    m.pos = c.a.idx_out;
    if (const int st = run_kth_long(c.a, rows, c.kt, s)) return st;
    HIP_TRY(launch_tkm_apply(c.a, m, nullptr, rows, c.kt, s));
    return LABSORT_OK;
}

int labsort_topk_mask_workspace_status(const void *d_ws, void *stream) { return labsort_kth_workspace_status(d_ws, stream); }

uint64_t labsort_top_p_weight(uint32_t word, int key_type) {
    if (key_type == LABSORT_KEY_F32) return tp_weight_f32(word);
    if (key_type == LABSORT_KEY_BF16) return tp_weight_f32((word & 0xFFFFu) << 16);
    if (key_type == LABSORT_KEY_F16) return tp_weight_f16(word);
    return 0;
}

size_t labsort_top_p_workspace_bytes(size_t rows, size_t cols) { return tp_layout(rows, cols).total; }

int labsort_top_p_device(const void *d_keys, size_t rows, size_t cols, float p, const float *d_p, int key_type,
                         uint32_t fill_bits, void *d_keys_out, uint8_t *d_mask_out, uint32_t *d_kept_out, void *d_ws,
                         size_t ws_bytes, void *stream) {
    if (rows == 0 || cols == 0) return LABSORT_OK;
    if (!d_keys || (!d_keys_out && !d_mask_out && !d_kept_out)) return LABSORT_ERR_ARG;
    if (key_type != LABSORT_KEY_F32 && !key_type_is16(key_type)) return LABSORT_ERR_ARG;
    if (!d_p && !(p > 0.0f && p <= 1.0f)) return LABSORT_ERR_ARG;  // (a NaN fails both)
    if (cols > TP_MAX_COLS || rows > (size_t)0x7FFFFFFFu / cols) return LABSORT_ERR_ARG;
    const bool k16 = key_type_is16(key_type);
    const size_t esz = k16 ? 2 : 4;  // bytes per key
    if (k16 && ((((uintptr_t)d_keys | (uintptr_t)d_keys_out) & 1u) || (fill_bits >> 16))) return LABSORT_ERR_ARG;
    if (((uintptr_t)d_kept_out | (uintptr_t)d_p) & 3u) return LABSORT_ERR_ARG;
    // the one alias: the keys written over the input, element for element
    const size_t key_bytes = rows * cols * esz, mask_bytes = rows * cols, w_bytes = rows * 4;
    const struct {
        const void *at;
        size_t bytes;
    } r[5] = {{d_keys, key_bytes}, {d_keys_out, key_bytes}, {d_mask_out, mask_bytes}, {d_kept_out, w_bytes}, {d_p, w_bytes}};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) {
            if (!r[i].at || !r[j].at || (i == 0 && j == 1 && d_keys_out == d_keys)) continue;
            if (ranges_overlap(r[i].at, r[i].bytes, r[j].at, r[j].bytes)) return LABSORT_ERR_ARG;
        }
    const TpLayout L = tp_layout(rows, cols);
    if (!d_ws || ws_bytes < L.total) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    KthCall c = kth_call(d_keys, cols, 1, nullptr, 1, key_type, d_ws, KthLayout{});
    TkmArgs m{};
    m.keys_out = d_keys_out;
    m.mask_out = d_mask_out;
    m.fill = fill_bits;
    TpArgs tp{};
    tp.d_p = d_p;
    tp.p = p;
    tp.kept_out = d_kept_out;
    HIP_TRY(launch_zero(ws, L.zero_bytes, s));
    TimingScope ts(LABSORT_K_TOPK, s);
    if (cols <= (size_t)KTH_ROW_KEYS) {
        HIP_TRY(launch_tp_short(c.a, m, tp, rows, c.kt, s));
        return LABSORT_OK;
    }
    c.a.nch = (uint32_t)L.nch;
    c.a.st = reinterpret_cast<KthState *>(ws + L.off_st);
    c.a.keys_out = ws + L.off_key;
    c.a.idx_out = reinterpret_cast<uint32_t *>(ws + L.off_pos);
    m.pos = c.a.idx_out;
    tp.hist = reinterpret_cast<tp_mass_t *>(ws + L.off_hist);
    tp.st = reinterpret_cast<TpState *>(ws + L.off_tst);
    tp.cmass = reinterpret_cast<tp_mass_t *>(ws + L.off_cmass);
    return run_tp_long(c.a, m, tp, rows, c.kt, s);
}

int labsort_top_p_workspace_status(const void *d_ws, void *stream) { return labsort_kth_workspace_status(d_ws, stream); }

size_t labsort_sample_workspace_bytes(size_t rows, size_t cols, size_t ndraw) { return smp_layout(rows, cols, ndraw).total; }

int labsort_sample_device(const void *d_keys, size_t rows, size_t cols, const uint32_t *d_u, size_t ndraw, int key_type,
                          uint32_t *d_idx_out, void *d_ws, size_t ws_bytes, void *stream) {
    if (rows == 0 || cols == 0 || ndraw == 0) return LABSORT_OK;
    if (!d_keys || !d_u || !d_idx_out) return LABSORT_ERR_ARG;
    if (key_type != LABSORT_KEY_F32 && !key_type_is16(key_type)) return LABSORT_ERR_ARG;
    if (cols > TP_MAX_COLS || rows > (size_t)0x7FFFFFFFu / cols || rows > (size_t)0x7FFFFFFFu / ndraw) return LABSORT_ERR_ARG;
    const bool k16 = key_type_is16(key_type);
    if (k16 && ((uintptr_t)d_keys & 1u)) return LABSORT_ERR_ARG;
    if (((uintptr_t)d_u | (uintptr_t)d_idx_out) & 3u) return LABSORT_ERR_ARG;
    const size_t key_bytes = rows * cols * (k16 ? 2 : 4), w_bytes = rows * ndraw * 4;
    if (ranges_overlap(d_keys, key_bytes, d_u, w_bytes) || ranges_overlap(d_keys, key_bytes, d_idx_out, w_bytes) ||
        ranges_overlap(d_u, w_bytes, d_idx_out, w_bytes))
        return LABSORT_ERR_ARG;
    const SmpLayout L = smp_layout(rows, cols, ndraw);
    if (!d_ws || ws_bytes < L.total) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    KthCall c = kth_call(d_keys, cols, 1, nullptr, 1, key_type, d_ws, KthLayout{});
    SmpArgs sm{};
    sm.u = d_u;
    sm.idx_out = d_idx_out;
    sm.ndraw = (uint32_t)ndraw;
    HIP_TRY(launch_zero(ws, KTH_HDR_BYTES, s));
    TimingScope ts(LABSORT_K_TOPK, s);
    if (cols <= (size_t)KTH_ROW_KEYS) {
        HIP_TRY(launch_smp_short(c.a, sm, rows, c.kt, s));
        return LABSORT_OK;
    }
    c.a.nch = (uint32_t)L.nch;
    sm.cmass = reinterpret_cast<uint64_t *>(ws + L.off_cmass);
    sm.draw = reinterpret_cast<SmpDraw *>(ws + L.off_draw);
    return run_smp_long(c.a, sm, rows, c.kt, s);
}

int labsort_sample_workspace_status(const void *d_ws, void *stream) { return labsort_kth_workspace_status(d_ws, stream); }

}  // extern "C"
