// rowsort.hip -- dense row sort with positions (labsort_sort_rows_device): every row of a
// rows x cols matrix sorted stably, ascending or descending, keys of 32 or 16 bits, with or
// without the positions within the row (torch.sort(x, dim=-1)).  Top-k's contract with k = cols.
//
// Every row has the same length, so the segmented sort's length class is a host decision and the
// row index gives the base: no offsets, no class lists, no binning.  A row that fits the LDS tile
// is read once, sorted by the class bodies of lds_class.h and written once; a key's position is
// the slot it was loaded into, never read from memory:
//   32-bit keys with positions   the key/value shapes, v[j] = slot, carried through LDS as a payload
//   32-bit keys alone            the keys-only shapes
//   16-bit keys                  one packed word per key in the keys-only shapes,
//                                w = ((ord16(key) ^ x16) << 16) | slot with x16 = descending ? 0xFFFF : 0,
//                                sorted with flip = 0 on digits 2 and 3 only: the passes are stable LSD
//                                and the slots start in position order, so the low half needs no pass.
//                                Padding is 0xFFFFFFFF: it starts behind every key and ties at most with
//                                NaN images (ascending) on both digits, so it stays behind them.
// Longer rows (and 32-bit keys with positions past the pair tile) go to labsort_topk_device with
// k = cols on the caller's workspace.
#include <cstdlib>
#include <cstring>

#include "devutil.h"
#include "host.h"
#include "lds_class.h"
#include "segsort.h"
#include "sort16.h"
#include "topk.h"

namespace labsort {

namespace {

// What a key is: a 32-bit word ordered by (word ^ flip), a float32 word ordered by
// (f32_ord(word) ^ flip), or a 16-bit float packed with its position (above).
enum RsMode : int { RS_K32, RS_F32, RS_P16 };

// The key policy of lds_class.h.  x16, nan_t: of a 16-bit call (above).
template <int MODE>
struct RowKeys {
    const void *in;
    void *out;
    uint32_t *iout;  // nullptr for a 16-bit call without positions (uniform over the launch)
    uint32_t x16, nan_t;
    // the sorted word of element i, at position pos of its row
    __device__ __forceinline__ uint32_t load(size_t i, uint32_t pos) const {
        if constexpr (MODE == RS_P16) return ((ord16(static_cast<const uint16_t *>(in)[i], nan_t) ^ x16) << 16) | pos;
        else if constexpr (MODE == RS_F32) return f32_ord(static_cast<const uint32_t *>(in)[i]);
        else return static_cast<const uint32_t *>(in)[i];
    }
    // a key's position is the slot it was loaded into, never read from memory
    __device__ __forceinline__ uint32_t payload(size_t, uint32_t pos) const { return pos; }
    // element i of the outputs: the key untransformed, the position as a 32-bit word
    __device__ __forceinline__ void store_key(size_t i, uint32_t k) const {
        if constexpr (MODE == RS_P16) static_cast<uint16_t *>(out)[i] = (uint16_t)unord16((k >> 16) ^ x16);
        else static_cast<uint32_t *>(out)[i] = MODE == RS_F32 ? f32_unord(k) : k;
    }
    template <bool KV>
    __device__ __forceinline__ void store_payload(size_t i, uint32_t k, uint32_t v) const {
        static_assert(!(MODE == RS_P16 && KV), "a packed word carries its position");
        if constexpr (MODE == RS_P16) {
            if (iout) iout[i] = k & 0xFFFFu;
        } else if constexpr (KV) {
            iout[i] = v;
        }
    }
    // the digits that can differ: a packed word's position half never starts a pass
    static __device__ __forceinline__ uint32_t diff(uint32_t d) { return MODE == RS_P16 ? d & 0xFFFF0000u : d; }
};

// wave classes: one wave64 per row, wave-private LDS, no workgroup barrier (k_seg_wave on row = unit).
// fx: the flip of a 32-bit call, x16 of a 16-bit one (which sorts with flip = 0)
template <int KPT, bool KV, int MODE>
__global__ __launch_bounds__(SEG_WAVE_WPB * WAVE) void k_rs_wave(const void *in, void *out, uint32_t *iout, uint32_t rows,
                                                                 uint32_t len, uint32_t fx, uint32_t nan_t) {
    constexpr uint32_t CAP = WAVE * KPT;
    __shared__ WaveSmem<KPT, KV> sm_all[SEG_WAVE_WPB];
    const uint32_t lane = threadIdx.x & 63u, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t first = blockIdx.x * SEG_WAVE_WPB + wid;
    if (first >= rows || len == 0u || len > CAP) return;  // (wave-uniform; the host picks the class by len)
    WaveSmem<KPT, KV> &sm = sm_all[wid];
    const uint32_t flip = MODE == RS_P16 ? 0u : fx;
    const uint32_t sentinel = ~flip;
    const RowKeys<MODE> io{in, out, iout, MODE == RS_P16 ? fx : 0u, nan_t};
    const bool atomic_rank = lds_lane_ordered(sm.probe, lane);
    const uint32_t jn = (len + WAVE - 1u) / WAVE;  // 64-key groups that hold keys (<= KPT)
    for (uint32_t row = first; row < rows; row += gridDim.x * SEG_WAVE_WPB) {
        const size_t b = (size_t)row * len;
        if (len <= (uint32_t)WAVE) {
            // one key per lane: its stable rank is the count of keys before it in (key, lane) order
            const bool ok = lane < len;
            const uint32_t x = ok ? (io.load(b + (ok ? lane : 0u), lane) ^ flip) : 0xFFFFFFFFu;
            const uint32_t r = wave_rank64(x, len, lane);
            if (ok) {  // r < len
                io.store_key(b + r, x ^ flip);
                io.template store_payload<KV>(b + r, x ^ flip, lane);
            }
            continue;
        }
        uint32_t k[KPT];
        uint32_t v[KV ? KPT : 1];
        uint32_t a = ~0u, o = 0u;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t idx = (uint32_t)j * WAVE + lane;
            const bool ok = idx < len;
            k[j] = sentinel;
            if (ok) k[j] = io.load(b + idx, idx);
            if constexpr (KV) v[j] = idx;
            const uint32_t x = k[j] ^ flip;
            a &= ok ? x : ~0u;
            o |= ok ? x : 0u;
        }
        wave_and_or(a, o);
        const uint32_t diff = RowKeys<MODE>::diff(__builtin_amdgcn_readfirstlane(a ^ o));
        for (int pass = 0; pass < 4; ++pass) {
            const uint32_t shift = pass * 8;
            if (((diff >> shift) & 0xFFu) == 0u) continue;  // uniform over the row
#pragma unroll
            for (int q = 0; q < 4; ++q) sm.hist[q * WAVE + lane] = 0u;
            __builtin_amdgcn_wave_barrier();
            uint32_t rank[KPT];
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                rank[j] = 0u;
                if ((uint32_t)j < jn)  // wave-uniform; a group past the end holds padding only
                    rank[j] = rank8(sm.hist, ((k[j] ^ flip) >> shift) & 0xFFu, lane, atomic_rank);
            }
            __builtin_amdgcn_wave_barrier();
            {  // exclusive scan of the 256 counters: four per lane, then across the wave
                uint32_t c[4], s = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c[q] = sm.hist[4u * lane + q];
                    s += c[q];
                }
                uint32_t xs = s;  // (wave_incl_scan, written out: through the helper this kernel's instruction text moves)
#pragma unroll
                for (int offx = 1; offx < 64; offx <<= 1) {
                    const uint32_t t = __shfl_up(xs, offx);
                    if (lane >= (uint32_t)offx) xs += t;
                }
                uint32_t run = xs - s;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    sm.hist[4u * lane + q] = run;
                    run += c[q];
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if ((uint32_t)j < jn) rank[j] += sm.hist[((k[j] ^ flip) >> shift) & 0xFFu];  // < 64 jn <= CAP
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if ((uint32_t)j < jn) {
                    sm.keys[rank[j]] = k[j];
                    if constexpr (KV) sm.vals[rank[j]] = v[j];
                }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if ((uint32_t)j < jn) {
                    k[j] = sm.keys[(uint32_t)j * WAVE + lane];
                    if constexpr (KV) v[j] = sm.vals[(uint32_t)j * WAVE + lane];
                }
            __builtin_amdgcn_wave_barrier();
        }
        // padding sorts behind every key (stable, largest digits), so slots < len hold the keys
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t idx = (uint32_t)j * WAVE + lane;
            uint32_t vj = 0u;
            if constexpr (KV) vj = v[j];
            if (idx < len) {
                io.store_key(b + idx, k[j]);
                io.template store_payload<KV>(b + idx, k[j], vj);
            }
        }
    }
}

// block and tile classes: block_sort_unit (lds_class.h) on one row per workgroup
template <int BLOCK, int KPT, bool KV, int WPE, int MODE>
__global__ __launch_bounds__(BLOCK, WPE) void k_rs_block(const void *in, void *out, uint32_t *iout, uint32_t rows, uint32_t len,
                                                          uint32_t fx, uint32_t nan_t) {
    using S = TsSmem<BLOCK, KPT, KV>;
    constexpr int W = S::W;
    constexpr uint32_t TILE = S::TILE;
    static_assert(MODE != RS_P16 || TILE <= 65536u, "a position fits the packed word's low half");
    __shared__ S sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (blockIdx.x >= rows || len == 0u || len > TILE) return;  // (uniform; the host picks the class by len)
    const uint32_t flip = MODE == RS_P16 ? 0u : fx;
    const RowKeys<MODE> io{in, out, iout, MODE == RS_P16 ? fx : 0u, nan_t};
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    __syncthreads();
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        // (the row's stripe is formed again for every row, from a copy of len the compiler cannot
        // see through: hoisted out of the loop its values were held in SGPRs across it and spilled)
        uint32_t rl = len;
        asm volatile("" : "+s"(rl));
        block_sort_unit(sm, io, (size_t)row * len, block_stripe<W>(rl, lane, wid), flip, atomic_rank, lane, wid);
    }
}

// One launch: the kernel of class c over all rows.  Two grid forms: the segmented sort's fixed
// multiples of the CU count (what stays resident per CU) with a row loop, never more units than
// rows; or one wave / workgroup per row.  By measurement at 2^28 keys with positions (DESIGN.md
// §3.12, profiles/rowsort.txt; time of a unit per row over time of the fixed grid): the 512-key
// wave class (0.79-0.98) and the block class (0.89-0.94) take a unit per row, the 256-key wave
// class (1.01-1.09) and the tile class (1.01-1.04) the fixed grid; the 1024-key wave class showed
// no consistent winner (0.94-1.03) and keeps the fixed grid.  LABSORT_ROWSORT_GRID=rows / fixed
// forces one form for every class (harness/rowsort_bench.py's A/B, tests).
enum RsGrid : int { RS_GRID_AUTO, RS_GRID_ROWS, RS_GRID_FIXED };
template <int MODE, bool KV>
hipError_t launch_rs(int c, const void *in, void *out, uint32_t *iout, size_t rows, size_t cols, uint32_t fx,
                     uint32_t nan_t, int form, hipStream_t s) {
    const bool per_row = form == RS_GRID_ROWS || (form == RS_GRID_AUTO && (c == 1 || c == 3));
    const size_t cus = (size_t)cu_count();
    return seg_class_dispatch(c, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        constexpr SegClass g = SEG_CLASS[C];
        constexpr int KPT = KV ? g.kpt_kv : g.kpt;
        const size_t wgs = C < 3 ? (rows + SEG_WAVE_WPB - 1) / SEG_WAVE_WPB : rows;  // workgroups that have a row
        const size_t fixed = cus * (size_t)(KV ? g.wgs_kv : g.wgs);
        const unsigned grid = (unsigned)((per_row || wgs < fixed) ? wgs : fixed);
        if constexpr (C < 3)
            k_rs_wave<KPT, KV, MODE><<<grid, g.block, 0, s>>>(in, out, iout, (uint32_t)rows, (uint32_t)cols, fx, nan_t);
        else
            k_rs_block<g.block, KPT, KV, g.wpe, MODE><<<grid, g.block, 0, s>>>(in, out, iout, (uint32_t)rows, (uint32_t)cols, fx, nan_t);
        return hipGetLastError();
    });
}

// Which rows the LDS kernels take: the keys-only tile for packed 16-bit keys and for 32-bit keys
// without positions, the pair tile for 32-bit keys with positions.
bool rs_lds_path(size_t cols, bool k16, bool idx) {
    return cols <= ((k16 || !idx) ? (size_t)SEG_TILE_KEYS : (size_t)SEG_TILE_PAIRS);
}

}  // namespace

// The LDS path behind the entry's checks (also labsort_sort16_device's short rows, sort16.h)
int sort_rows_lds(const void *d_keys, size_t rows, size_t cols, int descending, int key_type, void *d_keys_out,
                  uint32_t *d_idx_out, void *d_ws, hipStream_t s) {
    const bool k16 = key_type_is16(key_type);
    HIP_TRY(launch_zero(d_ws, SEG_HDR_BYTES, s));  // (a kernel: graph-replayable; nothing sets the header after it)
    TimingScope ts(LABSORT_K_SEGSORT, s);
    const int c = seg_class_of(cols);
    int form = RS_GRID_AUTO;  // the grid form: per class, unless forced
    if (const char *e = std::getenv("LABSORT_ROWSORT_GRID"))
        form = !std::strcmp(e, "rows") ? RS_GRID_ROWS : !std::strcmp(e, "fixed") ? RS_GRID_FIXED : RS_GRID_AUTO;
    if (k16) {
        HIP_TRY((launch_rs<RS_P16, false>(c, d_keys, d_keys_out, d_idx_out, rows, cols, descending ? 0xFFFFu : 0u,
                                          nan_t16(key_type), form, s)));
        return LABSORT_OK;
    }
    const uint32_t flip = flip_of(key_type) ^ (descending ? 0xFFFFFFFFu : 0u);
    const bool f32 = key_type == LABSORT_KEY_F32;
    if (d_idx_out) {
        if (f32) HIP_TRY((launch_rs<RS_F32, true>(c, d_keys, d_keys_out, d_idx_out, rows, cols, flip, 0u, form, s)));
        else HIP_TRY((launch_rs<RS_K32, true>(c, d_keys, d_keys_out, d_idx_out, rows, cols, flip, 0u, form, s)));
    } else {
        if (f32) HIP_TRY((launch_rs<RS_F32, false>(c, d_keys, d_keys_out, nullptr, rows, cols, flip, 0u, form, s)));
        else HIP_TRY((launch_rs<RS_K32, false>(c, d_keys, d_keys_out, nullptr, rows, cols, flip, 0u, form, s)));
    }
    return LABSORT_OK;
}

}  // namespace labsort

using namespace labsort;

extern "C" {

size_t labsort_sort_rows_workspace_bytes(size_t rows, size_t cols) {
    if (rows == 0 || cols <= (size_t)SEG_TILE_PAIRS) return SEG_HDR_BYTES;
    return labsort_topk_workspace_bytes(rows, cols, cols);
}

int labsort_sort_rows_device(const void *d_keys, size_t rows, size_t cols, int descending, int key_type, void *d_keys_out,
                             uint32_t *d_idx_out, void *d_ws, size_t ws_bytes, void *stream) {
    static_assert(TK_HDR_BYTES == SEG_HDR_BYTES, "one header, one status word, on both paths");
    if (rows == 0 || cols == 0) return LABSORT_OK;
    if (!topk_key_type_ok(key_type)) return LABSORT_ERR_ARG;
    if (const int rc = dense_rows_args(d_keys, rows, cols, cols, key_type, d_keys_out, d_idx_out)) return rc;
    const bool k16 = key_type_is16(key_type);
    if (!d_ws || ws_bytes < labsort_sort_rows_workspace_bytes(rows, cols)) return LABSORT_ERR_ARG;
    if (!rs_lds_path(cols, k16, d_idx_out != nullptr))
        return labsort_topk_device(d_keys, rows, cols, cols, descending, key_type, d_keys_out, d_idx_out, d_ws, ws_bytes,
                                   stream);
    return sort_rows_lds(d_keys, rows, cols, descending, key_type, d_keys_out, d_idx_out, d_ws, as_stream(stream));
}

int labsort_sort_rows_workspace_status(const void *d_ws, void *stream) {
    // word 0 of the header: cleared and never set on the LDS path, top-k's error word on the long one
    return labsort_topk_workspace_status(d_ws, stream);
}

}  // extern "C"
