// sort16.hip -- sort of bfloat16 / float16 rows of any length (labsort_sort16_device): the dense row
// sort's contract for the 16-bit key types, with a path of its own for rows longer than the LDS tile.
//
// Rows that fit the tile go to the row sort's LDS kernels (rowsort.hip, sort_rows_lds).  A longer row
// is sorted on u = ord16(key) ^ x16 (x16 = descending ? 0xFFFF : 0) by two stable LSD passes with
// 8-bit digits, low byte then high byte, over 2-byte keys and 4-byte positions:
//   pass 1 reads the input and writes u and, with positions, where each key was loaded from, to a
//          temporary in the workspace;
//   pass 2 reads the temporary and writes unord16(u ^ x16) and the positions to the outputs.
// Rows are independent and cut into chunks of up to S16_CHUNK consecutive keys.  A pass is three
// launches, none of which waits for another workgroup:
//   count    one workgroup per (row, chunk) counts the pass's digit in LDS and stores its 256 counts
//            to the table cnt[row][digit][chunk] (plain stores: the table is a function of the keys);
//   scan     an exclusive scan along the chunk axis of every (row, digit), in place, and the row's
//            256 digit totals; one thread or one workgroup per (row, digit), chosen by the host from
//            the chunks per row;
//   scatter  one workgroup per (row, chunk): the digit bases from the row's totals, its keys ranked
//            stably by digit (the lane-ordered wave ranking of devutil.h, per-wave counters folded
//            as in lds_pass.h), keys and positions reordered in LDS so that a digit's run leaves
//            as consecutive elements, lane-consecutive 2- and 4-byte stores.
// The table serves both passes.  Without positions none is stored or loaded anywhere.
#include "devutil.h"
#include "host.h"
#include "segsort.h"
#include "sort16.h"
#include "topk.h"

namespace labsort {

namespace {

constexpr int S16_W = S16_BLOCK / WAVE;
constexpr uint32_t S16_KPW = (uint32_t)WAVE * S16_KPT;  // keys of a chunk that one wave ranks: a contiguous stripe

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
    __shared__ uint32_t h[256 * S16_SLOTS];
    constexpr uint32_t shift = FIRST ? 0u : 8u;
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / a.nch, chunk = blockIdx.x - row * a.nch;
    slot_hist_clear<S16_SLOTS, S16_BLOCK>(h, tid);
    __syncthreads();
    const uint16_t *base = a.kin + (size_t)row * a.cols;
    const uint32_t beg = chunk * (uint32_t)S16_CHUNK;
    const uint32_t end = a.cols - beg > (uint32_t)S16_CHUNK ? beg + (uint32_t)S16_CHUNK : a.cols;
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
                if ((vm[t] >> j) & 1u) slot_hist_add<S16_SLOTS>(h, (u[t][j] >> shift) & 255u, tid);
    }
    __syncthreads();
    if (tid < 256u) a.cnt[((size_t)row * 256u + tid) * a.nch + chunk] = slot_hist_fold<S16_SLOTS>(h, tid);
}

// scan, few chunks per row: thread i walks the nch words of (row, digit) i = row * 256 + digit
__global__ __launch_bounds__(256) void k_s16_scan_serial(uint32_t *cnt, uint32_t *tot, uint32_t nrd, uint32_t nch) {
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

// scan, many chunks per row: workgroup i scans the nch words of (row, digit) i in steps of its width
__global__ __launch_bounds__(S16_SCAN_BLOCK) void k_s16_scan_block(uint32_t *cnt, uint32_t *tot, uint32_t nch) {
    constexpr int NW = S16_SCAN_BLOCK / WAVE;
    __shared__ uint32_t wsum[NW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t *p = cnt + (size_t)blockIdx.x * nch;
    uint32_t carry = 0u;
    for (uint32_t c0 = 0; c0 < nch; c0 += (uint32_t)S16_SCAN_BLOCK) {  // (uniform over the workgroup)
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

// What a key carries through LDS beside itself: in pass 1 its place in the chunk (16 bits: its
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
    const uint32_t row = blockIdx.x / a.nch, chunk = blockIdx.x - row * a.nch;
    const size_t rowoff = (size_t)row * a.cols;
    const uint16_t *base = a.kin + rowoff;
    const uint32_t beg = chunk * (uint32_t)S16_CHUNK;
    const uint32_t n = a.cols - beg > (uint32_t)S16_CHUNK ? (uint32_t)S16_CHUNK : a.cols - beg;  // 1 .. S16_CHUNK
    const uint32_t end = beg + n;
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
    // digit d = tid: the row's total and what the chunks before this one hold of it
    uint32_t tot = 0u, pre = 0u;
    if (tid < 256u) {
        tot = a.tot[(size_t)row * 256u + tid];
        pre = a.cnt[((size_t)row * 256u + tid) * a.nch + chunk];
    }
    const uint32_t dbase = block_excl_scan<S16_BLOCK, 256>(tot, sm.wsum2);
    __syncthreads();  // the chunk is in LDS, the probe's answer is published
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    // wave wid ranks slots ws0 .. ws0 + S16_KPW - 1, slot ws0 + j * 64 + lane in k[j]: in order of
    // position over (wave, j, lane).  Slots from n on are padding, u = 0xFFFF: digit 255 in both
    // passes and behind every key, so the first n slots of the digit order hold the keys.
    const uint32_t ws0 = wid * S16_KPW;
    uint32_t ng = ws0 < n ? (n - ws0 + 63u) / 64u : 0u;  // 64-key groups of this wave that hold keys (wave-uniform)
    if (ng > (uint32_t)S16_KPT) ng = S16_KPT;
    uint32_t *wh = sm.whist + wid * 256u;
    for (uint32_t i = lane; i < 256u; i += WAVE) wh[i] = 0u;
    uint32_t k[S16_KPT];
    uint32_t v[(IDX && !FIRST) ? S16_KPT : 1];
#pragma unroll
    for (int j = 0; j < S16_KPT; ++j) {
        const uint32_t i = ws0 + (uint32_t)j * WAVE + lane;
        k[j] = i < n ? (uint32_t)sm.keys[i] : 0xFFFFu;
        if constexpr (IDX && !FIRST) v[j] = i < n ? a.pin[rowoff + beg + i] : 0u;
    }
    uint32_t rank[S16_KPT / 2] = {};
#pragma unroll
    for (int j = 0; j < S16_KPT; ++j) {
        uint32_t r = 0u;
        if ((uint32_t)j < ng) r = rank8(wh, (k[j] >> shift) & 0xFFu, lane, atomic_rank);
        set16(rank, j, r);
    }
    __syncthreads();  // every wave's counters are complete, sm.keys has been read
    const DigitSpan sp = fold_digit_offsets<S16_BLOCK, S16_W>(sm.whist, sm.wsum);
    if (tid < 256u) sm.goff[tid] = dbase + pre - sp.start;  // (mod 2^32: goff[d] + slot >= 0 for slot >= sp.start)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < S16_KPT; ++j) set16(rank, j, wh[(k[j] >> shift) & 0xFFu] + get16(rank, j));
#pragma unroll
    for (int j = 0; j < S16_KPT; ++j)
        if ((uint32_t)j < ng) {  // (ranked slots number the keys and the padding of the last group: dst < S16_CHUNK)
            const uint32_t dst = get16(rank, j);
            sm.keys[dst] = (uint16_t)k[j];
            if constexpr (IDX && FIRST) reinterpret_cast<uint16_t *>(sm.pay)[dst] = (uint16_t)(ws0 + (uint32_t)j * WAVE + lane);
            if constexpr (IDX && !FIRST) sm.pay[dst] = v[j];
        }
    __syncthreads();
    // slot i of the digit order: consecutive slots of one digit are consecutive elements of the row
    for (uint32_t i = tid; i < n; i += S16_BLOCK) {
        const uint32_t u = sm.keys[i];
        const uint32_t o = sm.goff[(u >> shift) & 0xFFu] + i;
        if (o >= a.cols) continue;  // (cannot happen while the count and the scatter read the same keys)
        uint16_t *kp = a.kout + rowoff + o;
        const uint32_t w = FIRST ? u : unord16(u ^ a.x16);
        if constexpr (S16_PAIR != 0) {
            // 4-byte stores where two neighbours of a run start 4-byte aligned: the even element stores
            // for both, the odd one only at the start of its run
            const uint32_t d = (u >> shift) & 0xFFu;
            if ((((uintptr_t)kp >> 1) & 1u) == 0u) {
                const uint32_t u2 = i + 1u < n ? (uint32_t)sm.keys[i + 1u] : ~u;
                if (i + 1u < n && o + 1u < a.cols && ((u2 >> shift) & 0xFFu) == d)
                    *reinterpret_cast<uint32_t *>(kp) = w | ((FIRST ? u2 : unord16(u2 ^ a.x16)) << 16);
                else
                    *kp = (uint16_t)w;
            } else if (i == 0u || (((uint32_t)sm.keys[i - 1u] >> shift) & 0xFFu) != d) {
                *kp = (uint16_t)w;
            }
        } else {
            *kp = (uint16_t)w;
        }
        if constexpr (IDX && FIRST) a.pout[rowoff + o] = beg + reinterpret_cast<const uint16_t *>(sm.pay)[i];
        if constexpr (IDX && !FIRST) a.pout[rowoff + o] = sm.pay[i];
    }
}

inline size_t s16_chunks(size_t cols) { return (cols + S16_CHUNK - 1) / S16_CHUNK; }

struct S16Layout {
    size_t off_cnt, off_tot, off_keys, off_pos, total;
};
S16Layout s16_layout(size_t rows, size_t cols, bool idx) {
    S16Layout L;
    Carver c;
    c.take(SEG_HDR_BYTES);
    L.off_cnt = c.take(rows * 256 * s16_chunks(cols) * sizeof(uint32_t));
    L.off_tot = c.take(rows * 256 * sizeof(uint32_t));
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
    const uint32_t nrd = (uint32_t)(rows * 256);
    if (a.nch <= S16_SCAN_SERIAL) k_s16_scan_serial<<<(nrd + 255u) / 256u, 256, 0, s>>>(a.cnt, a.tot, nrd, a.nch);
    else k_s16_scan_block<<<nrd, S16_SCAN_BLOCK, 0, s>>>(a.cnt, a.tot, a.nch);
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
    a.cnt = reinterpret_cast<uint32_t *>(ws + L.off_cnt);
    a.tot = reinterpret_cast<uint32_t *>(ws + L.off_tot);
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
