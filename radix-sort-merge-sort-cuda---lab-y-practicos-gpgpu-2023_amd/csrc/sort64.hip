// sort64.hip -- sort of rows of 8-byte keys of any length (labsort_sort64_device): the dense row
// sort's contract for uint64, int64 and float64 keys.
//
// Everything orders u = image(key) ^ x64 (x64 = descending ? ~0 : 0) as a uint64 by stable LSD
// passes with 8-bit digits, and runs only the passes whose digit varies, which the device decides
// from the OR of u and the OR of ~u over the keys: bit b varies where both have it.
//   cols <= S64_CHUNK  one workgroup per row (k_s64_row): the row into registers as u, the two ORs
//                      reduced over the workgroup, the varying bytes as passes through LDS, the row
//                      written once.  A key's position is the slot it was loaded into.  256, 512 or
//                      S64_BLOCK threads, the fewest whose S64_KPT keys each hold the row.
//   longer rows        cut into chunks of up to S64_CHUNK consecutive keys.  k_s64_bits ORs u and ~u
//                      of every chunk into two plan words, k_s64_plan writes the plan of the call
//                      (sort64.h, S64Plan), then for each byte p the three launches of chunk_pass.h --
//                      count, scan, scatter -- each of which reads the plan and returns if pass p is
//                      inactive, and k_s64_same, which works only when no pass is active.  The
//                      first active pass reads the input and maps it, the last one maps back; the
//                      passes between carry u and the positions through the outputs and the
//                      temporaries in turn, so that the last one lands in the outputs.
// No kernel waits on another workgroup.  Without positions none is stored or loaded anywhere.
#include "chunk_pass.h"
#include "devutil.h"
#include "host.h"
#include "segsort.h"
#include "sort64.h"
#include "topk.h"

namespace labsort {

namespace {

constexpr int S64_W = S64_BLOCK / WAVE;

struct S64Args {
    const uint64_t *kin;  // the input
    uint64_t *kout;       // the outputs
    uint32_t *pout;       // (with positions)
    uint64_t *tk;         // the temporaries (long path)
    uint32_t *tp;         // (with positions)
    uint32_t *cnt;        // [row][digit][chunk]: counts, after the scan the exclusive sums along the chunks
    uint32_t *tot;        // [row][digit]
    S64Plan *plan;
    uint32_t *hdr;        // the workspace's header
    uint64_t x64;
    uint32_t cols, nch;
    int kt;
};

// ---------------------------------------------------------------------------------
// short rows: one workgroup of BLOCK threads per row of up to BLOCK * S64_KPT keys
// ---------------------------------------------------------------------------------
template <bool IDX, int BLOCK>
struct S64RowSmem {
    uint64_t keys[BLOCK * S64_KPT];            // the row in the digit order of the pass
    uint16_t pay[IDX ? BLOCK * S64_KPT : 1];   // the slots the keys were loaded into
    uint32_t whist[BLOCK / WAVE * 256];
    uint32_t wsum[BLOCK / WAVE];
    uint64_t red[2 * (BLOCK / WAVE)];
    uint32_t probe[WAVE];
    uint32_t ordered;
};

template <bool IDX, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_s64_row(S64Args a) {
    static_assert(BLOCK % 256 == 0 && BLOCK <= S64_BLOCK, "256 threads hold the digits; a row is at most a chunk");
    constexpr int W = BLOCK / WAVE;
    __shared__ S64RowSmem<IDX, BLOCK> sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t rowoff = (size_t)blockIdx.x * a.cols;
    const uint32_t n = a.cols;  // 1 .. BLOCK * S64_KPT
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    // the row into registers (chunk_pass.h, WaveStripe); the padding is u = ~0
    const WaveStripe<S64_KPT> w(wid, n);
    using Carry = std::conditional_t<IDX, uint16_t, NoCarry>;
    uint64_t k[S64_KPT];
    uint32_t v[IDX ? S64_KPT : 1];
    uint64_t ou = 0ull, on = 0ull;
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = w.slot(j, lane);
        k[j] = ~0ull;
        if (i < n) {
            k[j] = key64_ord(a.kin[rowoff + i], a.kt) ^ a.x64;
            ou |= k[j];
            on |= ~k[j];
        }
        if constexpr (IDX) v[j] = i;
    }
    block_or2<W>(ou, on, sm.red, lane, wid);  // (its barrier publishes the probe's answer too)
    const uint64_t vary = ou & on;
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    for (uint32_t p = 0; p < 8u; ++p) {  // (uniform over the workgroup)
        const uint32_t shift = 8u * p;
        if (((vary >> shift) & 0xFFull) == 0ull) continue;
        uint32_t rank[S64_KPT / 2] = {};
        chunk_rank<BLOCK>(k, shift, w.ng, sm.whist, sm.wsum, rank, atomic_rank, lane, wid);
        __syncthreads();
        chunk_reorder<false>(k, v, shift, w.ng, sm.whist + wid * 256u, rank, sm.keys, reinterpret_cast<Carry *>(sm.pay));
        __syncthreads();
#pragma unroll
        for (int j = 0; j < S64_KPT; ++j)
            if ((uint32_t)j < w.ng) {
                const uint32_t i = w.slot(j, lane);
                k[j] = sm.keys[i];
                if constexpr (IDX) v[j] = sm.pay[i];
            }
        // (the next pass writes sm.keys behind two barriers, its counters are the wave's own)
    }
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = w.slot(j, lane);
        if (i < n) {
            a.kout[rowoff + i] = key64_unord(k[j] ^ a.x64, a.kt);
            if constexpr (IDX) a.pout[rowoff + i] = v[j];
        }
    }
}

// ---------------------------------------------------------------------------------
// long rows: the plan
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(S64_BLOCK) void k_s64_bits(S64Args a) {
    __shared__ uint64_t red[2 * S64_W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const Chunk c = chunk_of<S64_CHUNK>(a.cols, a.nch);
    const uint64_t *base = a.kin + c.rowoff + c.beg;
    uint64_t ou = 0ull, on = 0ull;
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = (uint32_t)j * S64_BLOCK + tid;
        if (i < c.n) {
            const uint64_t u = key64_ord(base[i], a.kt) ^ a.x64;
            ou |= u;
            on |= ~u;
        }
    }
    block_or2<S64_W>(ou, on, red, lane, wid);
    // The words only grow, so a workgroup whose bits a (possibly stale) read already shows adds
    // nothing: after the first few chunks of random keys almost none has to (one row of 2^27 keys:
    // 0.41 ms with every workgroup's pair of atomics on the same two words, 0.27 ms with the skip).
    if (tid == 0u) {
        if (ou & ~__hip_atomic_load(&a.plan->or_u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicOr(&a.plan->or_u, (unsigned long long)ou);
        if (on & ~__hip_atomic_load(&a.plan->or_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicOr(&a.plan->or_n, (unsigned long long)on);
    }
}

__global__ __launch_bounds__(WAVE) void k_s64_plan(S64Plan *pl, uint32_t *hdr) {
    if (threadIdx.x != 0u) return;
    const uint64_t vary = pl->or_u & pl->or_n;
    uint32_t mask = 0u, m = 0u;
    for (uint32_t p = 0; p < 8u; ++p)
        if ((vary >> (8u * p)) & 0xFFull) {
            mask |= 1u << p;
            ++m;
        }
    uint32_t j = 0u, prev = S64_IN;
    for (uint32_t p = 0; p < 8u; ++p) {
        const bool act = (mask >> p) & 1u;
        const uint32_t dst = ((m - 1u - j) & 1u) ? S64_TMP : S64_OUT;
        pl->src[p] = act ? prev : S64_IN;
        pl->dst[p] = act ? dst : S64_OUT;
        pl->last[p] = act && j == m - 1u ? 1u : 0u;
        if (act) {
            prev = dst;
            ++j;
        }
    }
    pl->mask = mask;
    pl->m = m;
    hdr[S64_HDR_MASK] = mask;
}

// what pass p reads and writes, from the plan (uniform over the grid)
struct S64Pass {
    const uint64_t *ks;
    const uint32_t *ps;
    uint64_t *kd;
    uint32_t *pd;
    bool first, last;
};
__device__ __forceinline__ S64Pass s64_pass(const S64Args &a, uint32_t p) {
    const uint32_t src = a.plan->src[p], dst = a.plan->dst[p];
    S64Pass q;
    q.first = src == S64_IN;
    q.last = a.plan->last[p] != 0u;
    q.ks = q.first ? a.kin : src == S64_OUT ? a.kout : a.tk;
    q.ps = src == S64_OUT ? a.pout : a.tp;
    q.kd = dst == S64_OUT ? a.kout : a.tk;
    q.pd = dst == S64_OUT ? a.pout : a.tp;
    return q;
}
// does pass p run?  (the gate of chunk_pass.h's scan, and of the count and the scatter)
struct S64Gate {
    const S64Plan *plan;
    uint32_t p;
    __device__ __forceinline__ bool operator()() const { return (plan->mask >> p) & 1u; }
};

// ---------------------------------------------------------------------------------
// long rows: a pass
// ---------------------------------------------------------------------------------
// count: digit p of the chunk's keys
__global__ __launch_bounds__(S64_BLOCK) void k_s64_count(S64Args a, uint32_t p) {
    if (!S64Gate{a.plan, p}()) return;
    __shared__ uint32_t h[256 * CP_SLOTS];
    const S64Pass q = s64_pass(a, p);
    const uint32_t shift = 8u * p, tid = threadIdx.x;
    const Chunk c = chunk_of<S64_CHUNK>(a.cols, a.nch);
    slot_hist_clear<CP_SLOTS, S64_BLOCK>(h, tid);
    __syncthreads();
    const uint64_t *base = q.ks + c.rowoff + c.beg;
    uint64_t u[S64_KPT];
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = (uint32_t)j * S64_BLOCK + tid;
        u[j] = i < c.n ? base[i] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = (uint32_t)j * S64_BLOCK + tid;
        if (i < c.n) slot_hist_add<CP_SLOTS>(h, digit_of(q.first ? key64_ord(u[j], a.kt) ^ a.x64 : u[j], shift), tid);
    }
    __syncthreads();
    if (tid < 256u) a.cnt[chunk_cnt_at(c, tid, a.nch)] = slot_hist_fold<CP_SLOTS>(h, tid);
}

template <bool IDX>
struct S64Smem {
    uint64_t keys[S64_CHUNK];           // the chunk in digit order
    uint32_t pay[IDX ? S64_CHUNK : 1];  // the keys' positions
    uint32_t whist[S64_W * 256];
    uint32_t wsum[S64_W];
    uint32_t wsum2[S64_W];
    uint32_t goff[256];  // digit d's keys of this chunk go to row elements goff[d] + (slot in digit order)
    uint32_t probe[WAVE];
    uint32_t ordered;
};

template <bool IDX>
__global__ __launch_bounds__(S64_BLOCK) void k_s64_scatter(S64Args a, uint32_t p) {
    if (!S64Gate{a.plan, p}()) return;
    __shared__ S64Smem<IDX> sm;
    const S64Pass q = s64_pass(a, p);
    const uint32_t shift = 8u * p;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Chunk c = chunk_of<S64_CHUNK>(a.cols, a.nch);
    const uint32_t n = c.n;
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    // the chunk into registers (chunk_pass.h, WaveStripe): slot i is element beg + i of the row, read
    // here and held across the reorder; the padding is u = ~0
    const WaveStripe<S64_KPT> w(wid, n);
    using Carry = std::conditional_t<IDX, uint32_t, NoCarry>;
    const uint64_t *kbase = q.ks + c.rowoff + c.beg;
    const uint32_t *pbase = q.ps + c.rowoff + c.beg;  // (read only in a later pass with positions)
    uint64_t k[S64_KPT];
    uint32_t v[IDX ? S64_KPT : 1];
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = w.slot(j, lane);
        k[j] = i < n ? kbase[i] : ~0ull;
        if constexpr (IDX) v[j] = q.first ? c.beg + i : i < n ? pbase[i] : 0u;
    }
    if (q.first) {
#pragma unroll
        for (int j = 0; j < S64_KPT; ++j) {
            if (w.slot(j, lane) < n) k[j] = key64_ord(k[j], a.kt) ^ a.x64;
        }
    }
    const uint32_t dbase = chunk_digit_base<S64_BLOCK>(a.cnt, a.tot, c, a.nch, sm.wsum2);
    __syncthreads();  // the probe's answer is published
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    uint32_t rank[S64_KPT / 2] = {};
    const DigitSpan sp = chunk_rank<S64_BLOCK>(k, shift, w.ng, sm.whist, sm.wsum, rank, atomic_rank, lane, wid);
    if (tid < 256u) sm.goff[tid] = dbase - sp.start;  // (mod 2^32: goff[d] + slot >= 0 for slot >= sp.start)
    __syncthreads();
    chunk_reorder<false>(k, v, shift, w.ng, sm.whist + wid * 256u, rank, sm.keys, reinterpret_cast<Carry *>(sm.pay));
    __syncthreads();
    // slot i of the digit order: consecutive slots of one digit are consecutive elements of the row
    uint64_t *kd = q.kd + c.rowoff;
    uint32_t *pd = q.pd + c.rowoff;
    chunk_store<S64_BLOCK>(sm.keys, sm.goff, shift, n, a.cols, [&](uint32_t i, uint64_t u, uint32_t o) {
        kd[o] = q.last ? key64_unord(u ^ a.x64, a.kt) : u;
        if constexpr (IDX) pd[o] = sm.pay[i];
    });
}

// every key of the call has one image (m == 0): the input in place, NaNs canonical
template <bool IDX>
__global__ __launch_bounds__(S64_BLOCK) void k_s64_same(S64Args a) {
    if (a.plan->m != 0u) return;
    const Chunk c = chunk_of<S64_CHUNK>(a.cols, a.nch);
#pragma unroll
    for (int j = 0; j < S64_KPT; ++j) {
        const uint32_t i = (uint32_t)j * S64_BLOCK + threadIdx.x;
        if (i < c.n) {
            const size_t e = c.rowoff + c.beg + i;
            a.kout[e] = key64_unord(key64_ord(a.kin[e], a.kt), a.kt);
            if constexpr (IDX) a.pout[e] = c.beg + i;
        }
    }
}

inline size_t s64_chunks(size_t cols) { return (cols + S64_CHUNK - 1) / S64_CHUNK; }
inline bool s64_row_path(size_t cols) { return cols <= (size_t)S64_CHUNK; }

// a row of up to S64_CHUNK keys: the smallest workgroup of the three whose registers hold it
template <bool IDX>
hipError_t s64_launch_row(const S64Args &a, size_t rows, hipStream_t s) {
    const unsigned grid = (unsigned)rows;
    if (S64_BLOCK > 256 && a.cols <= 256u * S64_KPT) k_s64_row<IDX, 256><<<grid, 256, 0, s>>>(a);
    else if (S64_BLOCK > 512 && a.cols <= 512u * S64_KPT) k_s64_row<IDX, (S64_BLOCK > 512 ? 512 : S64_BLOCK)><<<grid, 512, 0, s>>>(a);
    else k_s64_row<IDX, S64_BLOCK><<<grid, S64_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

struct S64Layout {
    ChunkTable t;
    size_t off_plan, off_keys, off_pos, total;
};
S64Layout s64_layout(size_t rows, size_t cols, bool idx) {
    S64Layout L;
    Carver c;
    c.take(SEG_HDR_BYTES);
    L.off_plan = c.take(S64_PLAN_BYTES);
    L.t = carve_chunk_table(c, rows, s64_chunks(cols));
    L.off_keys = c.take(rows * cols * 8);
    L.off_pos = idx ? c.take(rows * cols * 4) : 0;
    L.total = c.o;
    return L;
}

}  // namespace

}  // namespace labsort

using namespace labsort;

extern "C" {

uint64_t labsort_key_order_bits64(uint64_t word, int key_type) { return key64_ord(word, key_type); }
uint64_t labsort_key_from_order_bits64(uint64_t bits, int key_type) { return key64_unord(bits, key_type); }

size_t labsort_sort64_chunk_keys(void) { return (size_t)S64_CHUNK; }

size_t labsort_sort64_workspace_bytes(size_t rows, size_t cols, int with_positions) {
    if (rows == 0 || s64_row_path(cols)) return SEG_HDR_BYTES;
    return s64_layout(rows, cols, with_positions != 0).total;
}

int labsort_sort64_device(const void *d_keys, size_t rows, size_t cols, int descending, int key_type, void *d_keys_out,
                          uint32_t *d_idx_out, void *d_ws, size_t ws_bytes, void *stream) {
    static_assert(TK_HDR_BYTES == SEG_HDR_BYTES, "one header, one status word, for every dense entry");
    static_assert(S64_HDR_MASK * 4 < SEG_HDR_BYTES, "a word of the header");
    if (rows == 0 || cols == 0) return LABSORT_OK;
    if (!key_type_is64(key_type)) return LABSORT_ERR_ARG;
    if (const int rc = dense_rows_args(d_keys, rows, cols, cols, key_type, d_keys_out, d_idx_out)) return rc;
    const bool idx = d_idx_out != nullptr;
    if (!d_ws || ws_bytes < labsort_sort64_workspace_bytes(rows, cols, idx)) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    S64Args a = {};
    a.kin = static_cast<const uint64_t *>(d_keys);
    a.kout = static_cast<uint64_t *>(d_keys_out);
    a.pout = d_idx_out;
    a.hdr = reinterpret_cast<uint32_t *>(ws);
    a.x64 = descending ? ~0ull : 0ull;
    a.cols = (uint32_t)cols;
    a.kt = key_type;
    if (s64_row_path(cols)) {
        HIP_TRY(launch_zero(d_ws, SEG_HDR_BYTES, s));  // (a kernel: graph-replayable; nothing sets the header after it)
        TimingScope ts(LABSORT_K_SEGSORT, s);
        a.nch = 1u;
        HIP_TRY(idx ? s64_launch_row<true>(a, rows, s) : s64_launch_row<false>(a, rows, s));
        return LABSORT_OK;
    }
    const S64Layout L = s64_layout(rows, cols, idx);
    static_assert(SEG_HDR_BYTES == 256, "the plan lies directly behind the header: one clearing launch");
    HIP_TRY(launch_zero(d_ws, SEG_HDR_BYTES + S64_PLAN_BYTES, s));
    TimingScope ts(LABSORT_K_SEGSORT, s);
    a.plan = reinterpret_cast<S64Plan *>(ws + L.off_plan);
    a.cnt = reinterpret_cast<uint32_t *>(ws + L.t.off_cnt);
    a.tot = reinterpret_cast<uint32_t *>(ws + L.t.off_tot);
    a.tk = reinterpret_cast<uint64_t *>(ws + L.off_keys);
    a.tp = idx ? reinterpret_cast<uint32_t *>(ws + L.off_pos) : nullptr;
    a.nch = (uint32_t)s64_chunks(cols);
    const unsigned grid = (unsigned)(rows * a.nch);
    k_s64_bits<<<grid, S64_BLOCK, 0, s>>>(a);
    k_s64_plan<<<1, WAVE, 0, s>>>(a.plan, a.hdr);
    for (uint32_t p = 0; p < 8u; ++p) {
        k_s64_count<<<grid, S64_BLOCK, 0, s>>>(a, p);
        launch_chunk_scan(a.cnt, a.tot, rows, a.nch, S64Gate{a.plan, p}, s);
        if (idx) k_s64_scatter<true><<<grid, S64_BLOCK, 0, s>>>(a, p);
        else k_s64_scatter<false><<<grid, S64_BLOCK, 0, s>>>(a, p);
        HIP_TRY(hipGetLastError());
    }
    if (idx) k_s64_same<true><<<grid, S64_BLOCK, 0, s>>>(a);
    else k_s64_same<false><<<grid, S64_BLOCK, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return LABSORT_OK;
}

int labsort_sort64_workspace_status(const void *d_ws, void *stream) {
    // word 0 of the header: cleared by the call and set by nothing on either path
    return labsort_topk_workspace_status(d_ws, stream);
}

int labsort_sort64_passes(const void *d_ws, void *stream) {
    uint32_t w[S64_HDR_MASK + 1] = {};
    if (const int st = read_ws_words(d_ws, w, (int)S64_HDR_MASK + 1, as_stream(stream))) return -st;
    return (int)(w[S64_HDR_MASK] & 0xFFu);
}

}  // extern "C"
