// unique.hip -- distinct keys with counts, first positions and inverse (labsort_unique_device).
//
// Two keys are one value when their order images are equal.  The default call sorts the keys
// stably with the library's own entries -- labsort_sort_pairs_device on a (key, iota) copy for
// 4-byte keys with positions, labsort_sort_device into a temporary without, labsort_sort64_device
// for 8-byte keys -- and then runs the run-edge passes of this file over the sorted array;
// LABSORT_UNIQUE_CONSECUTIVE runs the same passes over the input as it lies.  The passes:
//   k_uq_count   one workgroup per chunk of UQ_CHUNK consecutive elements: element i is a head if
//                i == 0 or image(key[i]) != image(key[i - 1]); the chunk's head count by a plain store
//   scan         chunk_pass.h's scan kernels on one line: exclusive sums of the chunk counts in
//                place, the total into *d_num_out
//   k_uq_write   the chunk's heads again, ranked by ballots and popcounts and one fold over the
//                waves; head keys and their places compacted in LDS and stored as consecutive
//                elements; every element's run number to d_inverse_out
//   k_uq_counts  run lengths from the differences of the runs' starts
// No kernel waits on another workgroup.  The launch sequence depends on the host arguments only.
#include <algorithm>

#include "chunk_pass.h"
#include "devutil.h"
#include "host.h"
#include "segsort.h"
#include "sort64.h"
#include "topk.h"
#include "unique.h"

namespace labsort {

namespace {

template <class K>
struct UqArgs {
    const K *keys;        // the sorted keys, or the input in consecutive mode
    const uint32_t *pos;  // position in the input of every sorted key; nullptr: element i is input i
    K *uniq;
    uint32_t *first, *inverse;  // (either may be nullptr)
    uint32_t *start;      // start[j]: index in `keys` of run j's head (nullptr without counts)
    uint32_t *cnt;        // per chunk: heads, after the scan the heads of the chunks before it
    uint32_t *hdr;
    uint32_t n, sorted_by;
    UqImage<K> im;
};

template <class K>
__device__ __forceinline__ K uq_shfl_up1(K v) {
    if constexpr (sizeof(K) == 4) {
        return __shfl_up(v, 1);
    } else {
        const uint32_t lo = __shfl_up((uint32_t)v, 1), hi = __shfl_up((uint32_t)(v >> 32), 1);
        return ((uint64_t)hi << 32) | lo;
    }
}

// The chunk's elements of this thread as images, u[g * E + k] = element i0(g) + k of the chunk with
// i0(g) = wid * UQ_WAVE_KEYS + g * 64 E + lane * E, and the mask of those that are heads.  A group
// inside the chunk is one 16-byte load where the array is 16-byte aligned; the last group of a
// partial chunk and an unaligned input are read element by element.  The element before a lane's
// first comes from the lane below; lane 0 reads it from memory, the chunk before included.  Must be
// called by every lane of the wave.
template <class K>
struct UqGroup {
    static constexpr int E = 16 / sizeof(K), G = UQ_KPT / E;
    static constexpr uint32_t EMASK = (1u << E) - 1u;
    __device__ static __forceinline__ uint32_t i0(uint32_t wid, uint32_t lane, int g) {
        return wid * (uint32_t)UQ_WAVE_KEYS + (uint32_t)g * (WAVE * E) + lane * E;
    }
};

template <class K>
__device__ __forceinline__ uint32_t uq_load_heads(const K *keys, uint32_t cbeg, uint32_t cn, const UqImage<K> &im, uint32_t lane,
                                                  uint32_t wid, K (&u)[UQ_KPT]) {
    using L = UqGroup<K>;
    constexpr int E = L::E;
    const bool al16 = ((uintptr_t)keys & 15u) == 0u;  // (cbeg is a multiple of UQ_CHUNK)
    const K *base = keys + cbeg;
    uint32_t heads = 0u;
#pragma unroll
    for (int g = 0; g < L::G; ++g) {
        const uint32_t i0 = L::i0(wid, lane, g);
        K x[E];
        if (al16 && i0 + E <= cn) {
            const uint4 v = *reinterpret_cast<const uint4 *>(base + i0);
            if constexpr (E == 4) {
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            } else {
                x[0] = ((uint64_t)v.y << 32) | v.x, x[1] = ((uint64_t)v.w << 32) | v.z;
            }
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) x[k] = i0 + k < cn ? base[i0 + k] : (K)0;
        }
#pragma unroll
        for (int k = 0; k < E; ++k) u[g * E + k] = im.ord(x[k]);
        K prev = uq_shfl_up1(u[g * E + E - 1]);
        if (lane == 0u && i0 < cn && cbeg + i0 > 0u) prev = im.ord(keys[(size_t)cbeg + i0 - 1u]);
#pragma unroll
        for (int k = 0; k < E; ++k)
            if (i0 + k < cn) {
                const bool h = cbeg + i0 + k == 0u || u[g * E + k] != (k ? u[g * E + k - 1] : prev);
                heads |= (h ? 1u : 0u) << (g * E + k);
            }
    }
    return heads;
}

__device__ __forceinline__ uint32_t uq_chunk_len(uint32_t n, uint32_t cbeg) {
    return n - cbeg > (uint32_t)UQ_CHUNK ? (uint32_t)UQ_CHUNK : n - cbeg;
}

// ---- count: the heads of every chunk
template <class K>
__global__ __launch_bounds__(UQ_BLOCK) void k_uq_count(UqArgs<K> a) {
    __shared__ uint32_t wsum[UQ_W];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t cbeg = blockIdx.x * (uint32_t)UQ_CHUNK, cn = uq_chunk_len(a.n, cbeg);
    K u[UQ_KPT];
    const uint32_t heads = uq_load_heads(a.keys, cbeg, cn, a.im, lane, wid, u);
    uint32_t wt = 0u;
#pragma unroll
    for (int j = 0; j < UQ_KPT; ++j) wt += (uint32_t)__popcll(__ballot((heads >> j) & 1u));
    if (lane == 0u) wsum[wid] = wt;
    __syncthreads();
    if (tid == 0u) {
        uint32_t t = 0u;
#pragma unroll
        for (int w = 0; w < UQ_W; ++w) t += wsum[w];
        a.cnt[blockIdx.x] = t;
        if (blockIdx.x == 0u) a.hdr[UQ_HDR_SORT] = a.sorted_by;
    }
}

// ---- write: distinct keys, first positions, run starts, inverse
template <class K>
struct UqSmem {
    K keys[UQ_CHUNK];        // the chunk's head images, compacted
    uint16_t loc[UQ_CHUNK];  // and their places in the chunk
    uint32_t wsum[UQ_W];
};

// E consecutive words from a 4 E-byte aligned address
template <int E>
__device__ __forceinline__ void uq_load_words(const uint32_t *p, uint32_t (&w)[E]) {
    if constexpr (E == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        w[0] = v.x, w[1] = v.y;
    }
}

template <class K>
__global__ __launch_bounds__(UQ_BLOCK) void k_uq_write(UqArgs<K> a) {
    using L = UqGroup<K>;
    constexpr int E = L::E;
    __shared__ UqSmem<K> sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t cbeg = blockIdx.x * (uint32_t)UQ_CHUNK, cn = uq_chunk_len(a.n, cbeg);
    K u[UQ_KPT];
    const uint32_t heads = uq_load_heads(a.keys, cbeg, cn, a.im, lane, wid, u);
    // pre[g]: the wave's heads in front of this lane's elements of group g -- the groups before, and
    // in this group the lanes below by one ballot per k; wt: the wave's heads
    uint32_t pre[L::G], wt = 0u;
#pragma unroll
    for (int g = 0; g < L::G; ++g) {
        uint32_t below = 0u, gt = 0u;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const uint64_t bal = __ballot((heads >> (g * E + k)) & 1u);
            below += mbcnt64(bal);
            gt += (uint32_t)__popcll(bal);
        }
        pre[g] = wt + below;
        wt += gt;
    }
    if (lane == 0u) sm.wsum[wid] = wt;
    __syncthreads();
    uint32_t wbase = 0u, ctot = 0u;
#pragma unroll
    for (int w = 0; w < UQ_W; ++w) {
        const uint32_t t = sm.wsum[w];
        if ((uint32_t)w < wid) wbase += t;
        ctot += t;
    }
    const uint32_t base = a.cnt[blockIdx.x];  // the heads of the chunks before this one
#pragma unroll
    for (int g = 0; g < L::G; ++g) {
        const uint32_t i0 = L::i0(wid, lane, g), hg = (heads >> (g * E)) & L::EMASK;
#pragma unroll
        for (int k = 0; k < E; ++k)
            if ((hg >> k) & 1u) {
                const uint32_t r = wbase + pre[g] + (uint32_t)__popc(hg & ((1u << k) - 1u));  // < ctot <= cn
                sm.keys[r] = u[g * E + k];
                sm.loc[r] = (uint16_t)(i0 + k);
            }
        if (a.inverse && i0 < cn) {
            // element i lies in run base + (heads up to and including i) - 1
            uint32_t p[E];
            if (a.pos) {
                if (i0 + E <= cn) uq_load_words<E>(a.pos + cbeg + i0, p);
                else
#pragma unroll
                    for (int k = 0; k < E; ++k) p[k] = i0 + k < cn ? a.pos[cbeg + i0 + k] : a.n;
            } else {
#pragma unroll
                for (int k = 0; k < E; ++k) p[k] = cbeg + i0 + k;
            }
#pragma unroll
            for (int k = 0; k < E; ++k)
                if (i0 + k < cn && p[k] < a.n)  // (a position is below n: the sort permutes an iota)
                    a.inverse[p[k]] = base + wbase + pre[g] + (uint32_t)__popc(hg & ((2u << k) - 1u)) - 1u;
        }
    }
    __syncthreads();
    for (uint32_t r = tid; r < ctot; r += UQ_BLOCK) {
        const uint32_t o = base + r, st = cbeg + sm.loc[r];
        if (o >= a.n) continue;  // (cannot happen while the count and the write read the same keys)
        a.uniq[o] = a.im.unord(sm.keys[r]);
        if (a.start) a.start[o] = st;
        if (a.first) a.first[o] = a.pos ? a.pos[st] : st;
    }
}

// ---- counts: run j is [start[j], start[j + 1]), the last one ends at n.  The grid is sized for n
// runs; a workgroup past the m that the scan left in *num returns.
__global__ __launch_bounds__(UQ_BLOCK) void k_uq_counts(const uint32_t *start, const uint32_t *num, uint32_t n, uint32_t *counts) {
    uint32_t m = *num;
    if (m > n) m = n;  // (cannot happen)
    const uint32_t j0 = blockIdx.x * (uint32_t)UQ_COUNTS_PER_WG;
    if (j0 >= m) return;
#pragma unroll
    for (int q = 0; q < UQ_COUNTS_PER_WG / UQ_BLOCK; ++q) {
        const uint32_t j = j0 + (uint32_t)q * UQ_BLOCK + threadIdx.x;
        if (j < m) counts[j] = (j + 1u < m ? start[j + 1u] : n) - start[j];
    }
}

// ---- the pair sort's input: tk = keys, tp = 0, 1, 2, ... (tk and tp 16-byte aligned)
__global__ __launch_bounds__(UQ_BLOCK) void k_uq_iota_copy(const uint32_t *in, uint32_t *tk, uint32_t *tp, uint32_t n) {
    const uint32_t i = (blockIdx.x * (uint32_t)UQ_BLOCK + threadIdx.x) * 4u;
    if (i >= n) return;
    if (i + 4u <= n) {
        uint4 v;
        if (((uintptr_t)in & 15u) == 0u) v = *reinterpret_cast<const uint4 *>(in + i);
        else v = make_uint4(in[i], in[i + 1u], in[i + 2u], in[i + 3u]);
        *reinterpret_cast<uint4 *>(tk + i) = v;
        *reinterpret_cast<uint4 *>(tp + i) = make_uint4(i, i + 1u, i + 2u, i + 3u);
    } else {
        for (uint32_t j = i; j < n; ++j) {
            tk[j] = in[j];
            tp[j] = j;
        }
    }
}

inline size_t uq_chunks(size_t n) { return (n + UQ_CHUNK - 1) / UQ_CHUNK; }
inline bool uq_key_type_ok(int kt) { return device_key_type_ok(kt) || key_type_is64(kt); }
inline size_t uq_max_keys(int kt) { return key_type_is64(kt) ? (size_t)0x7FFFFFFFu : labsort_max_keys(LABSORT_ALGO_RADIX); }

// The inner sort's workspace for n keys.  The sorts change algorithm at fixed sizes and a larger n
// may need less than a smaller one across such a size, so every size at which one of them does is
// asked too: the result never shrinks as n grows.
size_t uq_inner_need(size_t n, int kt, bool pos) {
    if (key_type_is64(kt)) return labsort_sort64_workspace_bytes(1, n, pos ? 1 : 0);
    return pos ? labsort_pairs_workspace_bytes(n, LABSORT_ALGO_AUTO) : labsort_workspace_bytes(n, LABSORT_ALGO_AUTO);
}
size_t uq_inner_bytes(size_t n, int kt, bool pos) {
    n = std::min(n, uq_max_keys(kt));  // (a call with more keys is rejected; the size keeps growing with n all the same)
    const size_t edges[] = {(size_t)TS_TILE_KV, (size_t)TS_TILE, (size_t)LABSORT_AUTO_MERGE_MAX_KEYS, GS_MIN_N,
                            (size_t)LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS, GS_MAX_N - 1, GS_MAX_N, HY_MIN_N, HY_MAX_N};
    size_t b = uq_inner_need(n, kt, pos);
    for (const size_t e : edges)
        for (size_t t = e > 0 ? e - 1 : 0; t <= e + 1 && t < n; ++t) b = std::max(b, uq_inner_need(t, kt, pos));
    return align_up(b, 256);
}

// header | the inner sort's workspace | sorted keys | their positions | chunk counts | run starts
struct UqLayout {
    size_t off_inner, inner_bytes, off_keys, off_pos, off_cnt, off_start, total;
};
UqLayout uq_layout(size_t n, int kt, bool consecutive, bool pos) {
    UqLayout L = {};
    Carver c;
    c.take(SEG_HDR_BYTES);
    if (!consecutive) {
        L.inner_bytes = uq_inner_bytes(n, kt, pos);
        L.off_inner = c.take(L.inner_bytes);
        L.off_keys = c.take(n * (key_type_is64(kt) ? 8 : 4));
        if (pos) L.off_pos = c.take(n * 4);
    }
    L.off_cnt = c.take(uq_chunks(n) * sizeof(uint32_t));
    L.off_start = c.take(n * 4);
    L.total = c.o;
    return L;
}

template <class K>
int uq_edge_passes(const K *keys, const uint32_t *pos, size_t n, int kt, uint32_t sorted_by, void *uniq, uint32_t *counts,
                   uint32_t *first, uint32_t *inverse, uint32_t *num, char *ws, const UqLayout &L, hipStream_t s) {
    TimingScope ts(LABSORT_K_SEGSORT, s);
    UqArgs<K> a = {};
    a.keys = keys;
    a.pos = pos;
    a.uniq = static_cast<K *>(uniq);
    a.first = first;
    a.inverse = inverse;
    a.start = counts ? reinterpret_cast<uint32_t *>(ws + L.off_start) : nullptr;
    a.cnt = reinterpret_cast<uint32_t *>(ws + L.off_cnt);
    a.hdr = reinterpret_cast<uint32_t *>(ws);
    a.n = (uint32_t)n;
    a.sorted_by = sorted_by;
    a.im = UqImage<K>{kt};
    const uint32_t nch = (uint32_t)uq_chunks(n);
    k_uq_count<K><<<nch, UQ_BLOCK, 0, s>>>(a);
    // chunk_pass.h's scan kernels on one line of nch words; its total is m
    if (nch <= CP_SCAN_SERIAL) k_chunk_scan_serial<<<1, 256, 0, s>>>(a.cnt, num, 1u, nch, AlwaysOn{});
    else k_chunk_scan_block<<<1, CP_SCAN_BLOCK, 0, s>>>(a.cnt, num, nch, AlwaysOn{});
    k_uq_write<K><<<nch, UQ_BLOCK, 0, s>>>(a);
    if (counts)
        k_uq_counts<<<(unsigned)((n + UQ_COUNTS_PER_WG - 1) / UQ_COUNTS_PER_WG), UQ_BLOCK, 0, s>>>(a.start, num, a.n, counts);
    HIP_TRY(hipGetLastError());
    return LABSORT_OK;
}

}  // namespace

}  // namespace labsort

using namespace labsort;

extern "C" {

size_t labsort_unique_chunk_keys(void) { return (size_t)UQ_CHUNK; }

size_t labsort_unique_workspace_bytes(size_t n, int key_type, int flags, int with_positions) {
    if (n == 0 || !uq_key_type_ok(key_type)) return SEG_HDR_BYTES;
    const bool consecutive = (flags & LABSORT_UNIQUE_CONSECUTIVE) != 0;
    const size_t without = uq_layout(n, key_type, consecutive, false).total;
    // (a workspace sized with positions serves a call without them)
    return with_positions ? std::max(without, uq_layout(n, key_type, consecutive, true).total) : without;
}

int labsort_unique_device(const void *d_keys, size_t n, int key_type, int flags, void *d_unique_out, uint32_t *d_counts_out,
                          uint32_t *d_first_out, uint32_t *d_inverse_out, uint32_t *d_num_out, void *d_ws, size_t ws_bytes,
                          void *stream) {
    static_assert(TK_HDR_BYTES == SEG_HDR_BYTES, "one header, one status word, for every dense entry");
    static_assert(UQ_HDR_SORT * 4 < SEG_HDR_BYTES, "a word of the header");
    if (!uq_key_type_ok(key_type) || (flags & ~LABSORT_UNIQUE_CONSECUTIVE)) return LABSORT_ERR_ARG;
    if (!d_unique_out || !d_num_out) return LABSORT_ERR_ARG;
    const bool wide = key_type_is64(key_type), consecutive = flags != 0;
    const size_t esz = wide ? 8 : 4;
    if ((((uintptr_t)d_keys | (uintptr_t)d_unique_out) & (esz - 1)) ||
        (((uintptr_t)d_counts_out | (uintptr_t)d_first_out | (uintptr_t)d_inverse_out | (uintptr_t)d_num_out) & 3u))
        return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_num_out, 0, sizeof(uint32_t), s));
        return LABSORT_OK;
    }
    if (!d_keys || n > uq_max_keys(key_type)) return LABSORT_ERR_ARG;
    // no output may share a byte with the input or with another output
    const struct {
        const void *p;
        size_t bytes;
    } buf[] = {{d_keys, n * esz}, {d_unique_out, n * esz}, {d_counts_out, n * 4}, {d_first_out, n * 4}, {d_inverse_out, n * 4},
               {d_num_out, 4}};
    for (size_t i = 0; i < sizeof(buf) / sizeof(buf[0]); ++i)
        for (size_t j = i + 1; j < sizeof(buf) / sizeof(buf[0]); ++j)
            if (buf[i].p && buf[j].p && ranges_overlap(buf[i].p, buf[i].bytes, buf[j].p, buf[j].bytes)) return LABSORT_ERR_ARG;
    const bool pos = d_first_out || d_inverse_out;
    if (!d_ws || ws_bytes < labsort_unique_workspace_bytes(n, key_type, flags, pos)) return LABSORT_ERR_ARG;
    char *ws = static_cast<char *>(d_ws);
    const UqLayout L = uq_layout(n, key_type, consecutive, pos);
    const void *sorted = d_keys;
    const uint32_t *tp = nullptr;
    uint32_t sorted_by = UQ_SORT_NONE;
    if (!consecutive) {
        void *tk = ws + L.off_keys, *inner = ws + L.off_inner;
        uint32_t *p = pos ? reinterpret_cast<uint32_t *>(ws + L.off_pos) : nullptr;
        int st;
        if (wide) {
            st = labsort_sort64_device(d_keys, 1, n, 0, key_type, tk, p, inner, L.inner_bytes, stream);
            sorted_by = UQ_SORT_64;
        } else if (pos) {
            {
                TimingScope ts(LABSORT_K_SEGSORT, s);
                k_uq_iota_copy<<<(unsigned)((n + 4 * UQ_BLOCK - 1) / (4 * UQ_BLOCK)), UQ_BLOCK, 0, s>>>(
                    static_cast<const uint32_t *>(d_keys), static_cast<uint32_t *>(tk), p, (uint32_t)n);
                HIP_TRY(hipGetLastError());
            }
            st = labsort_sort_pairs_device(tk, p, tk, p, n, key_type, LABSORT_ALGO_AUTO, inner, L.inner_bytes, stream);
            sorted_by = UQ_SORT_PAIRS;
        } else {
            st = labsort_sort_device(d_keys, tk, n, key_type, LABSORT_ALGO_AUTO, inner, L.inner_bytes, stream);
            sorted_by = UQ_SORT_KEYS;
        }
        if (st) return st;
        sorted = tk;
        tp = p;
    }
    if (wide)
        return uq_edge_passes(static_cast<const uint64_t *>(sorted), tp, n, key_type, sorted_by, d_unique_out, d_counts_out,
                              d_first_out, d_inverse_out, d_num_out, ws, L, s);
    return uq_edge_passes(static_cast<const uint32_t *>(sorted), tp, n, key_type, sorted_by, d_unique_out, d_counts_out, d_first_out,
                          d_inverse_out, d_num_out, ws, L, s);
}

int labsort_unique_workspace_status(const void *d_ws, size_t n, int key_type, int flags, void *stream) {
    hipStream_t s = as_stream(stream);
    if (n == 0 || (flags & LABSORT_UNIQUE_CONSECUTIVE) || !device_key_type_ok(key_type)) {
        HIP_TRY(hipStreamSynchronize(s));  // no sort ran, or one that reports nothing
        return LABSORT_OK;
    }
    uint32_t w[UQ_HDR_SORT + 1] = {};
    if (const int st = read_ws_words(d_ws, w, (int)UQ_HDR_SORT + 1, s)) return st;
    const void *inner = static_cast<const char *>(d_ws) + SEG_HDR_BYTES;  // (uq_layout: directly behind the header)
    if (w[UQ_HDR_SORT] == UQ_SORT_PAIRS) return labsort_pairs_workspace_status(inner, n, LABSORT_ALGO_AUTO, stream);
    if (w[UQ_HDR_SORT] == UQ_SORT_KEYS) return labsort_workspace_status(inner, n, LABSORT_ALGO_AUTO, stream);
    return LABSORT_OK;
}

}  // extern "C"
