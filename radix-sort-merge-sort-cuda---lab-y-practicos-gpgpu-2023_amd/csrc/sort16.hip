// sort16.hip -- sort of bfloat16 / float16 rows of any length (labsort_sort16_device): the dense row
// sort's contract for the 16-bit key types, with a path of its own for rows longer than the LDS tile.
//
// Rows that fit the tile go to the row sort's LDS kernels (rowsort.hip, sort_rows_lds).  A longer row
// is sorted on u = ord16(key) ^ x16 (x16 = descending ? 0xFFFF : 0) by two stable LSD passes with
// 8-bit digits, low byte then high byte, over 2-byte keys and 4-byte positions:
//   pass 1 reads the input and writes u and, with positions, where each key was loaded from, to a
//          temporary in the workspace;
//   pass 2 reads the temporary and writes unord16(u ^ x16) and the positions to the outputs.
// Rows are independent and cut into chunks of up to S16_CHUNK consecutive keys; a pass is the
// three launches of chunk_pass.h: count, scan (one thread or one workgroup per (row, digit), by
// the chunks per row), scatter (lane-consecutive 2- and 4-byte stores).
// The table serves both passes.  Without positions none is stored or loaded anywhere.
#include "chunk_pass.h"
#include "devutil.h"
#include "host.h"
#include "segsort.h"
#include "sort16.h"
#include "topk.h"

namespace labsort {

namespace {

constexpr int S16_W = S16_BLOCK / WAVE;

// FIRST: the element is a key of the input and becomes u; else it is u already (the temporary).
// Only the low half of x counts.
template <bool FIRST>
__device__ __forceinline__ uint32_t s16_u(uint32_t x, uint32_t nan_t, uint32_t x16) {
    if constexpr (FIRST) return ord16(x, nan_t) ^ x16;
    else return x & 0xFFFFu;
}

struct S16Args {
    const uint16_t *kin;  // pass 1: the input; pass 2: the temporary keys (u)
    const uint32_t *pin;  // pass 2 with positions: the temporary positions
    uint16_t *kout;
    uint32_t *pout;       // with positions
    uint32_t *cnt;        // [row][digit][chunk]: counts, after the scan the exclusive sums along the chunks
    uint32_t *tot;        // [row][digit]
    uint32_t cols, nch, nan_t, x16;
};

// Octs of the chunk [beg, end) of a row as u (devutil.h, load_group: the top-k select's loads)
template <bool FIRST>
__device__ __forceinline__ uint32_t s16_load(const S16Args &a, const uint16_t *base, uint32_t beg, uint32_t end, uint32_t mis,
                                             uint32_t q, uint32_t (&u)[8], int64_t &i0) {
    const uint32_t nan_t = a.nan_t, x16 = a.x16;
    return load_group(base, beg, end, mis, q, u, i0, [nan_t, x16](uint32_t x) { return s16_u<FIRST>(x, nan_t, x16); });
}

// count: digit (u >> shift) & 255 of the chunk's keys
template <bool FIRST>
__global__ __launch_bounds__(S16_BLOCK) void k_s16_count(S16Args a) {
    __shared__ uint32_t h[256 * CP_SLOTS];
    constexpr uint32_t shift = FIRST ? 0u : 8u;
    const uint32_t tid = threadIdx.x;
    const Chunk c = chunk_of<S16_CHUNK>(a.cols, a.nch);
    slot_hist_clear<CP_SLOTS, S16_BLOCK>(h, tid);
    __syncthreads();
    const uint16_t *base = a.kin + c.rowoff;
    const uint32_t beg = c.beg, end = beg + c.n;
    const uint32_t mis = group_mis(base, beg), nq = group_count<8>(beg, end, mis);
    for (uint32_t q0 = 0; q0 < nq; q0 += 2u * S16_BLOCK) {
        uint32_t u[2][8], vm[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t q = q0 + (uint32_t)t * S16_BLOCK + tid;
            int64_t i0;
            vm[t] = q < nq ? s16_load<FIRST>(a, base, beg, end, mis, q, u[t], i0) : 0u;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((vm[t] >> j) & 1u) slot_hist_add<CP_SLOTS>(h, digit_of(u[t][j], shift), tid);
    }
    __syncthreads();
    if (tid < 256u) a.cnt[chunk_cnt_at(c, tid, a.nch)] = slot_hist_fold<CP_SLOTS>(h, tid);
}

// pay: what a key carries through LDS beside itself: in pass 1 its place in the chunk (16 bits: its
// position is the chunk's first plus that, never read from memory), in pass 2 its position.
template <bool FIRST, bool IDX>
struct S16Smem {
    uint16_t keys[S16_CHUNK];  // the chunk as loaded, then in digit order
    uint32_t pay[IDX ? (FIRST ? S16_CHUNK / 2 : S16_CHUNK) : 1];
    uint32_t whist[S16_W * 256];
    uint32_t wsum[S16_W];
    uint32_t wsum2[S16_W];
    uint32_t goff[256];  // digit d's keys of this chunk go to row elements goff[d] + (slot in digit order)
    uint32_t probe[WAVE];
    uint32_t ordered;
};

template <bool FIRST, bool IDX>
__global__ __launch_bounds__(S16_BLOCK) void k_s16_scatter(S16Args a) {
    constexpr uint32_t shift = FIRST ? 0u : 8u;
    __shared__ S16Smem<FIRST, IDX> sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Chunk c = chunk_of<S16_CHUNK>(a.cols, a.nch);
    const size_t rowoff = c.rowoff;
    const uint16_t *base = a.kin + rowoff;
    const uint32_t beg = c.beg, n = c.n, end = beg + n;
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    {  // the chunk into LDS as 16-bit u, element beg + i in slot i
        const uint32_t mis = group_mis(base, beg), nq = group_count<8>(beg, end, mis);
        for (uint32_t q = tid; q < nq; q += S16_BLOCK) {
            uint32_t u[8];
            int64_t i0;
            const uint32_t vm = s16_load<FIRST>(a, base, beg, end, mis, q, u, i0);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((vm >> j) & 1u) sm.keys[(uint32_t)(i0 + j - (int64_t)beg)] = (uint16_t)u[j];  // < n
        }
    }
    const uint32_t dbase = chunk_digit_base<S16_BLOCK>(a.cnt, a.tot, c, a.nch, sm.wsum2);
    __syncthreads();  // the chunk is in LDS, the probe's answer is published
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    // the chunk into registers (chunk_pass.h, WaveStripe); the padding is u = 0xFFFF.  What a key
    // carries: in pass 1 its place in the chunk, in pass 2 its position.
    const WaveStripe<S16_KPT> w(wid, n);
    using Carry = std::conditional_t<!IDX, NoCarry, std::conditional_t<FIRST, uint16_t, uint32_t>>;
    uint32_t k[S16_KPT];
    uint32_t v[IDX ? S16_KPT : 1];
#pragma unroll
    for (int j = 0; j < S16_KPT; ++j) {
        const uint32_t i = w.slot(j, lane);
        k[j] = i < n ? (uint32_t)sm.keys[i] : 0xFFFFu;
        if constexpr (IDX && FIRST) v[j] = i;
        if constexpr (IDX && !FIRST) v[j] = i < n ? a.pin[rowoff + beg + i] : 0u;
    }
    uint32_t rank[S16_KPT / 2] = {};
    const DigitSpan sp = chunk_rank<S16_BLOCK>(k, shift, w.ng, sm.whist, sm.wsum, rank, atomic_rank, lane, wid);
    if (tid < 256u) sm.goff[tid] = dbase - sp.start;  // (mod 2^32: goff[d] + slot >= 0 for slot >= sp.start)
    __syncthreads();
    chunk_reorder<true>(k, v, shift, w.ng, sm.whist + wid * 256u, rank, sm.keys, reinterpret_cast<Carry *>(sm.pay));
    __syncthreads();
    // slot i of the digit order: consecutive slots of one digit are consecutive elements of the row
    chunk_store<S16_BLOCK>(sm.keys, sm.goff, shift, n, a.cols, [&](uint32_t i, uint32_t u, uint32_t o) {
        a.kout[rowoff + o] = (uint16_t)(FIRST ? u : unord16(u ^ a.x16));
        if constexpr (IDX && FIRST) a.pout[rowoff + o] = beg + reinterpret_cast<const uint16_t *>(sm.pay)[i];
        if constexpr (IDX && !FIRST) a.pout[rowoff + o] = sm.pay[i];
    });
}

inline size_t s16_chunks(size_t cols) { return (cols + S16_CHUNK - 1) / S16_CHUNK; }

struct S16Layout {
    ChunkTable t;
    size_t off_keys, off_pos, total;
};
S16Layout s16_layout(size_t rows, size_t cols, bool idx) {
    S16Layout L;
    Carver c;
    c.take(SEG_HDR_BYTES);
    L.t = carve_chunk_table(c, rows, s16_chunks(cols));
    L.off_keys = c.take(rows * cols * 2);
    L.off_pos = idx ? c.take(rows * cols * 4) : 0;
    L.total = c.o;
    return L;
}

bool s16_lds_path(size_t cols) { return cols <= (size_t)SEG_TILE_KEYS; }

template <bool FIRST>
hipError_t s16_pass(const S16Args &a, size_t rows, bool idx, hipStream_t s) {
    const unsigned grid = (unsigned)(rows * a.nch);
    k_s16_count<FIRST><<<grid, S16_BLOCK, 0, s>>>(a);
    launch_chunk_scan(a.cnt, a.tot, rows, a.nch, AlwaysOn{}, s);
    if (idx) k_s16_scatter<FIRST, true><<<grid, S16_BLOCK, 0, s>>>(a);
    else k_s16_scatter<FIRST, false><<<grid, S16_BLOCK, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

}  // namespace labsort

using namespace labsort;

extern "C" {

size_t labsort_sort16_chunk_keys(void) { return (size_t)S16_CHUNK; }

size_t labsort_sort16_workspace_bytes(size_t rows, size_t cols, int with_positions) {
    if (rows == 0 || s16_lds_path(cols)) return SEG_HDR_BYTES;
    return s16_layout(rows, cols, with_positions != 0).total;
}

int labsort_sort16_device(const void *d_keys, size_t rows, size_t cols, int descending, int key_type, void *d_keys_out,
                          uint32_t *d_idx_out, void *d_ws, size_t ws_bytes, void *stream) {
    static_assert(TK_HDR_BYTES == SEG_HDR_BYTES, "one header, one status word, for every dense entry");
    if (rows == 0 || cols == 0) return LABSORT_OK;
    if (!key_type_is16(key_type)) return LABSORT_ERR_ARG;
    if (const int rc = dense_rows_args(d_keys, rows, cols, cols, key_type, d_keys_out, d_idx_out)) return rc;
    const bool idx = d_idx_out != nullptr;
    if (!d_ws || ws_bytes < labsort_sort16_workspace_bytes(rows, cols, idx)) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    if (s16_lds_path(cols)) return sort_rows_lds(d_keys, rows, cols, descending, key_type, d_keys_out, d_idx_out, d_ws, s);
    const S16Layout L = s16_layout(rows, cols, idx);
    char *ws = static_cast<char *>(d_ws);
    HIP_TRY(launch_zero(d_ws, SEG_HDR_BYTES, s));  // (a kernel: graph-replayable; nothing sets the header after it)
    TimingScope ts(LABSORT_K_SEGSORT, s);
    uint16_t *tk = reinterpret_cast<uint16_t *>(ws + L.off_keys);
    uint32_t *tp = idx ? reinterpret_cast<uint32_t *>(ws + L.off_pos) : nullptr;
    S16Args a;
    a.cnt = reinterpret_cast<uint32_t *>(ws + L.t.off_cnt);
    a.tot = reinterpret_cast<uint32_t *>(ws + L.t.off_tot);
    a.cols = (uint32_t)cols;
    a.nch = (uint32_t)s16_chunks(cols);
    a.nan_t = nan_t16(key_type);
    a.x16 = descending ? 0xFFFFu : 0u;
    a.kin = static_cast<const uint16_t *>(d_keys);
    a.pin = nullptr;
    a.kout = tk;
    a.pout = tp;
    HIP_TRY(s16_pass<true>(a, rows, idx, s));
    a.kin = tk;
    a.pin = tp;
    a.kout = static_cast<uint16_t *>(d_keys_out);
    a.pout = d_idx_out;
    HIP_TRY(s16_pass<false>(a, rows, idx, s));
    return LABSORT_OK;
}

int labsort_sort16_workspace_status(const void *d_ws, void *stream) {
    // word 0 of the header: cleared by the call and set by nothing on either path
    return labsort_topk_workspace_status(d_ws, stream);
}

}  // extern "C"
