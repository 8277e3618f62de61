// search.hip -- ranks of values in sorted rows (labsort_searchsorted_device): torch.searchsorted and
// torch.bucketize under the library's order images.
//
// out[r][j] = the number of elements e of the row's sequence with u(e) < u(values[r][j]) (right:
// <=), u the order image.  Two paths, chosen by cols alone:
//   k_ss_lds     cols <= SS_LDS_BYTES / sizeof(key): a workgroup stages its sequence's images in LDS
//                once (through the sorter if there is one) and walks chunks of SS_CHUNK values; each
//                thread runs its SS_VPT searches side by side over the LDS array
//   k_ss_sample  longer sequences: SS_SAMPLES sample images per sequence, the last element of each of
//                SS_SAMPLES equal strides, into the workspace
//   k_ss_long    stages the sequence's samples in LDS, finds each value's stride there and finishes
//                inside that one stride in global memory, SS_VPT searches side by side
// Every search is ss_rank8: a descent over the powers of two below the sequence's length, so its
// number of probes is fixed by cols and every probe is clamped into the sequence, whatever the data.
// No kernel waits on another workgroup.  The launch sequence depends on the host arguments only.
//
// The same searches with counters as their sink (labsort_bucket_counts_device, and
// labsort_bincount_device without the search) follow behind them: k_bc_lds, k_bc_long, k_bincount.
#include <algorithm>

#include "devutil.h"
#include "host.h"
#include "search.h"
#include "segsort.h"

namespace labsort {

namespace {

template <class K, class Im>
struct SsArgs {
    const K *seq;            // seq_rows x cols
    const uint32_t *sorter;  // nullptr, or seq_rows x cols: element i in order is seq[sorter[i]]
    const K *vals;           // rows x nv values of rows x nv ranks
    uint32_t *out;
    K *table;                // long path: SS_SAMPLES images per sequence
    uint32_t *hdr;           // long path: the workspace's header
    uint32_t cols, nv;       // elements per sequence; values per row (all of them with one shared sequence)
    uint32_t slices;         // workgroups per row; workgroup s takes chunks s, s + slices, ...
    uint32_t per_row;        // 1: row r is searched in sequence r; 0: one row, one sequence
    uint32_t right;
    Im im;
};

// ---- 16 bytes as E = 16 / sizeof(K) key words and back
__device__ __forceinline__ void ss_unpack(const uint4 &v, uint16_t (&x)[8]) {
    x[0] = (uint16_t)v.x, x[1] = (uint16_t)(v.x >> 16), x[2] = (uint16_t)v.y, x[3] = (uint16_t)(v.y >> 16);
    x[4] = (uint16_t)v.z, x[5] = (uint16_t)(v.z >> 16), x[6] = (uint16_t)v.w, x[7] = (uint16_t)(v.w >> 16);
}
__device__ __forceinline__ void ss_unpack(const uint4 &v, uint32_t (&x)[4]) { x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w; }
__device__ __forceinline__ void ss_unpack(const uint4 &v, uint64_t (&x)[2]) {
    x[0] = ((uint64_t)v.y << 32) | v.x, x[1] = ((uint64_t)v.w << 32) | v.z;
}
__device__ __forceinline__ uint4 ss_pack(const uint16_t (&x)[8]) {
    return make_uint4(x[0] | ((uint32_t)x[1] << 16), x[2] | ((uint32_t)x[3] << 16), x[4] | ((uint32_t)x[5] << 16),
                      x[6] | ((uint32_t)x[7] << 16));
}
__device__ __forceinline__ uint4 ss_pack(const uint32_t (&x)[4]) { return make_uint4(x[0], x[1], x[2], x[3]); }
__device__ __forceinline__ uint4 ss_pack(const uint64_t (&x)[2]) {
    return make_uint4((uint32_t)x[0], (uint32_t)(x[0] >> 32), (uint32_t)x[1], (uint32_t)(x[1] >> 32));
}

__device__ __forceinline__ bool ss_al16(const void *p) { return ((uintptr_t)p & 15u) == 0u; }

// The image of element i (< cols) of a sequence in order; a sorter entry past the row is clamped
template <class K, class Im>
__device__ __forceinline__ K ss_elem(const K *seq, const uint32_t *sorter, uint32_t cols, const Im &im, uint32_t i) {
    uint32_t p = i;
    if (sorter) {
        p = sorter[i];
        p = p < cols ? p : cols - 1u;
    }
    return im.ord(seq[p]);
}

// ---- the search.  A sequence type gives at(j, p), the image at place p of value j's sequence, for
// any p (it clamps), and len(j) <= the len that `top` was taken from.  pos[j] becomes the largest
// count c <= len(j) found by the descent with every probed prefix satisfying e < v (right: e <= v):
// on an ascending sequence the number of such elements.  floor(log2(len)) + 1 probes per value.
__device__ __forceinline__ uint32_t ss_top(uint32_t len) { return len ? 1u << (31 - __clz((int)len)) : 0u; }

// REV: the sequence type hands out its elements last to first and pos[j] counts, from that end, the
// elements that do NOT satisfy the predicate (on an ascending sequence len(j) - pos[j] do).
template <bool REV, class K, class Seq>
__device__ __forceinline__ void ss_rank8(const Seq &q, uint32_t top, const K (&v)[SS_VPT], bool right, uint32_t (&pos)[SS_VPT]) {
#pragma unroll
    for (int j = 0; j < SS_VPT; ++j) pos[j] = 0u;
    for (uint32_t s = top; s != 0u; s >>= 1) {
        K e[SS_VPT];
#pragma unroll
        for (int j = 0; j < SS_VPT; ++j) e[j] = q.at(j, pos[j] + s - 1u);
#pragma unroll
        for (int j = 0; j < SS_VPT; ++j) {
            const bool below = e[j] < v[j] || (right && e[j] == v[j]);
            const bool take = pos[j] + s <= q.len(j) && below != REV;
            pos[j] += take ? s : 0u;
        }
    }
}

// n >= 1 images in LDS, one sequence for every value
template <class K>
struct SsLdsSeq {
    const K *img;
    uint32_t n;
    __device__ __forceinline__ K at(int, uint32_t p) const { return img[p < n ? p : n - 1u]; }
    __device__ __forceinline__ uint32_t len(int) const { return n; }
};

// For value j the elements start[j] .. start[j] + last[j] of a sequence in global memory, of which
// the first last[j] are searched (the one behind them is known, and is where a probe is clamped to),
// handed out last to first: place p is element start[j] + last[j] - 1 - p.  A stride of a power of
// two elements ends on a cache line's end, so the descent's probes p = s - 1, with s the large powers
// of two, are last elements of lines, and the small steps that follow a probe move down inside its
// line; first to last they would move up into the next line, one more line per value half the time.
template <class K, class Im>
struct SsStrideSeq {
    const K *seq;
    const uint32_t *sorter;
    uint32_t cols;
    Im im;
    uint32_t start[SS_VPT], last[SS_VPT];
    __device__ __forceinline__ K at(int j, uint32_t p) const {
        return ss_elem(seq, sorter, cols, im, start[j] + (p < last[j] ? last[j] - 1u - p : last[j]));
    }
    __device__ __forceinline__ uint32_t len(int j) const { return last[j]; }
};

// ---- the walk over a row's values: workgroup (row, slice) takes the row's chunks slice, slice +
// slices, ...; a thread loads its SS_VPT consecutive values by 16-byte loads where the row is
// 16-byte aligned and the values lie inside it, element by element otherwise, has `rank` turn their
// images into ranks and stores those the same way.  STRIPED (the long path, whose probes of global
// memory outweigh the values' own traffic): thread t owns values t, t + SS_BLOCK, ... of the chunk
// instead, loaded and stored element by element, so that one probe instruction of a wave serves 64
// consecutive values and values that come in order probe the same few cache lines.  No barrier inside.
template <bool STRIPED, class K, class Im, class Rank>
__device__ __forceinline__ void ss_walk(const SsArgs<K, Im> &a, uint32_t row, uint32_t slice, const Rank &rank) {
    constexpr int E = 16 / sizeof(K), G = SS_VPT / E;
    const K *vrow = a.vals + (size_t)row * a.nv;
    uint32_t *orow = a.out + (size_t)row * a.nv;
    const bool val16 = ss_al16(vrow), oal16 = ss_al16(orow);
    const uint32_t nch = (a.nv + (uint32_t)SS_CHUNK - 1u) / (uint32_t)SS_CHUNK;
    for (uint32_t c = slice; c < nch; c += a.slices) {
        if constexpr (STRIPED) {
            const uint32_t i0 = c * (uint32_t)SS_CHUNK + threadIdx.x;
            if (i0 >= a.nv) continue;
            K v[SS_VPT];
#pragma unroll
            for (int k = 0; k < SS_VPT; ++k) {
                const uint32_t i = i0 + (uint32_t)k * SS_BLOCK;
                v[k] = a.im.ord(i < a.nv ? vrow[i] : (K)0);
            }
            uint32_t pos[SS_VPT];
            rank(v, pos);
#pragma unroll
            for (int k = 0; k < SS_VPT; ++k) {
                const uint32_t i = i0 + (uint32_t)k * SS_BLOCK;
                if (i < a.nv) orow[i] = pos[k];
            }
            continue;
        }
        const uint32_t i0 = c * (uint32_t)SS_CHUNK + threadIdx.x * (uint32_t)SS_VPT;
        if (i0 >= a.nv) continue;
        const uint32_t left = a.nv - i0;  // >= 1
        const bool full = left >= (uint32_t)SS_VPT;
        K v[SS_VPT];
        if (val16 && full) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                K t[E];
                ss_unpack(reinterpret_cast<const uint4 *>(vrow + i0)[g], t);
#pragma unroll
                for (int k = 0; k < E; ++k) v[g * E + k] = t[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < SS_VPT; ++k) v[k] = (uint32_t)k < left ? vrow[i0 + k] : (K)0;
        }
#pragma unroll
        for (int k = 0; k < SS_VPT; ++k) v[k] = a.im.ord(v[k]);
        uint32_t pos[SS_VPT];
        rank(v, pos);
        if (oal16 && full) {
            reinterpret_cast<uint4 *>(orow + i0)[0] = make_uint4(pos[0], pos[1], pos[2], pos[3]);
            reinterpret_cast<uint4 *>(orow + i0)[1] = make_uint4(pos[4], pos[5], pos[6], pos[7]);
        } else {
#pragma unroll
            for (int k = 0; k < SS_VPT; ++k)
                if ((uint32_t)k < left) orow[i0 + k] = pos[k];
        }
    }
}

// ---- LDS path: 1 <= cols <= SS_LDS_BYTES / sizeof(K)
template <class K, class Im>
__global__ __launch_bounds__(SS_BLOCK) void k_ss_lds(SsArgs<K, Im> a) {
    constexpr int E = 16 / sizeof(K);
    __shared__ __attribute__((aligned(16))) K img[SS_LDS_BYTES / sizeof(K)];
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.slices, slice = blockIdx.x - row * a.slices;
    const size_t soff = a.per_row ? (size_t)row * a.cols : 0;
    const K *seq = a.seq + soff;
    const uint32_t *sorter = a.sorter ? a.sorter + soff : nullptr;
    if (!sorter && ss_al16(seq)) {
        const uint32_t groups = a.cols / (uint32_t)E;
        for (uint32_t g = tid; g < groups; g += SS_BLOCK) {
            K t[E];
            ss_unpack(reinterpret_cast<const uint4 *>(seq)[g], t);
#pragma unroll
            for (int k = 0; k < E; ++k) t[k] = a.im.ord(t[k]);
            reinterpret_cast<uint4 *>(img)[g] = ss_pack(t);
        }
        for (uint32_t i = groups * (uint32_t)E + tid; i < a.cols; i += SS_BLOCK) img[i] = a.im.ord(seq[i]);
    } else {
        for (uint32_t i = tid; i < a.cols; i += SS_BLOCK) img[i] = ss_elem(seq, sorter, a.cols, a.im, i);
    }
    __syncthreads();
    const SsLdsSeq<K> q = {img, a.cols};
    const uint32_t top = ss_top(a.cols);
    const bool right = a.right != 0u;
    ss_walk<false>(a, row, slice, [&](const K(&v)[SS_VPT], uint32_t(&pos)[SS_VPT]) { ss_rank8<false>(q, top, v, right, pos); });
}

// ---- long path: the samples
template <class K, class Im>
__global__ __launch_bounds__(SS_SAMPLE_BLOCK) void k_ss_sample(SsArgs<K, Im> a) {
    constexpr uint32_t PER = SS_SAMPLES / SS_SAMPLE_BLOCK;  // workgroups per sequence
    const uint32_t r = blockIdx.x / PER, j = (blockIdx.x - r * PER) * (uint32_t)SS_SAMPLE_BLOCK + threadIdx.x;
    const size_t soff = (size_t)r * a.cols;
    const unsigned long long end = (unsigned long long)(j + 1u) * ss_stride(a.cols);
    const uint32_t i = (end < a.cols ? (uint32_t)end : a.cols) - 1u;  // (an empty stride repeats the last element)
    a.table[(size_t)r * SS_SAMPLES + j] = ss_elem(a.seq + soff, a.sorter ? a.sorter + soff : nullptr, a.cols, a.im, i);
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.hdr[0] = 0u;  // the status word of every dense entry: clear
}

// ---- long path: the search.  c = the number of samples with e < v (right: e <= v) among the ns
// strides that hold an element: the strides before c lie below v whole, stride c ends on an element
// that does not, so the rank is c * stride + the count among the elements of stride c before its
// last; c == ns puts v behind everything.  The same predicate on both levels lands left and right on
// the two ends of a run that spans strides.
template <class K, class Im>
__global__ __launch_bounds__(SS_BLOCK) void k_ss_long(SsArgs<K, Im> a) {
    constexpr int E = 16 / sizeof(K);
    __shared__ __attribute__((aligned(16))) K img[SS_SAMPLES];
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.slices, slice = blockIdx.x - row * a.slices;
    const size_t soff = a.per_row ? (size_t)row * a.cols : 0;
    const K *table = a.table + (a.per_row ? (size_t)row * SS_SAMPLES : 0);  // (16-byte aligned: the workspace's regions)
    for (uint32_t g = tid; g < (uint32_t)(SS_SAMPLES / E); g += SS_BLOCK)
        reinterpret_cast<uint4 *>(img)[g] = reinterpret_cast<const uint4 *>(table)[g];
    __syncthreads();
    const uint32_t stride = ss_stride(a.cols), ns = ss_strides(a.cols);  // ns >= 1
    const SsLdsSeq<K> q = {img, ns};
    const uint32_t top1 = ss_top(ns), top2 = ss_top(stride - 1u), cols = a.cols;
    const bool right = a.right != 0u;
    SsStrideSeq<K, Im> g = {a.seq + soff, a.sorter ? a.sorter + soff : nullptr, cols, a.im, {}, {}};
    ss_walk<true>(a, row, slice, [&](const K(&v)[SS_VPT], uint32_t(&pos)[SS_VPT]) {
        uint32_t c[SS_VPT];
        ss_rank8<false>(q, top1, v, right, c);
#pragma unroll
        for (int j = 0; j < SS_VPT; ++j) {
            const uint32_t sj = c[j] < ns ? c[j] : ns - 1u;
            g.start[j] = sj * stride;  // < cols
            const uint32_t seg = cols - g.start[j] < stride ? cols - g.start[j] : stride;  // >= 1
            g.last[j] = seg - 1u;
        }
        ss_rank8<true>(g, top2, v, right, pos);  // (from the stride's end: pos counts the elements that do not)
#pragma unroll
        for (int j = 0; j < SS_VPT; ++j) pos[j] = c[j] >= ns ? cols : g.start[j] + g.last[j] - pos[j];
    });
}

// ======== counting: labsort_bucket_counts_device and labsort_bincount_device ========================
// The same searches with another sink: a rank is a bin, and a bin's counter is what gets written.
//   k_bc_lds    nedges <= bc_row_edges: images and nedges + 1 counters in LDS, LDS atomics in the walk,
//               the counters flushed to the row's output at the end (stored where the workgroup owns
//               the row, added by global atomics to the zeroed output where several share it)
//   k_bc_long   longer edge rows: k_ss_sample's table, k_ss_long's two-level search, global atomics
//   k_bincount  the bin is the value itself (past nbins: nbins); LDS counters up to BIN_ROW_BINS bins
// The walk is a second one (bc_walk) so that ss_walk and the k_ss_* kernels stay as they are.
template <class K, class Im>
struct BcArgs {
    const K *edges;       // edge_rows x nedges
    const K *vals;        // rows x nv
    uint32_t *out;        // rows x (nedges + 1) counters
    const K *table;       // long path: SS_SAMPLES images per edge row
    uint32_t nedges, nv;
    uint32_t slices;      // workgroups per row; workgroup s takes chunks s, s + slices, ...
    uint32_t per_row;     // 1: row r is counted on edge row r; 0: one edge row for every row
    uint32_t right;
    uint32_t store;       // LDS path: slices == 1, the flush stores (the output need not be zero)
    Im im;
};

// The ranks of a thread's n (1 .. SS_VPT) values into add(bin, count): one call per run of equal
// neighbours, which is one per thread where all values fall in one bin or come sorted
template <class Add>
__device__ __forceinline__ void bc_emit(const uint32_t (&pos)[SS_VPT], uint32_t n, const Add &add) {
    uint32_t run = 1u;
#pragma unroll
    for (int k = 0; k < SS_VPT; ++k) {
        if ((uint32_t)k < n) {
            const int k1 = k + 1 < SS_VPT ? k + 1 : k;
            if (LABSORT_BC_COMBINE != 0 && k1 != k && (uint32_t)k1 < n && pos[k1] == pos[k]) {
                ++run;
            } else {
                add(pos[k], run);
                run = 1u;
            }
        }
    }
}

// ss_walk's loads (16-byte where the row is 16-byte aligned; STRIPED: element by element, thread t
// the values t, t + SS_BLOCK, ... of a chunk) with bc_emit as the sink.  No barrier inside.
template <bool STRIPED, class K, class Im, class Rank, class Add>
__device__ __forceinline__ void bc_walk(const K *vrow, uint32_t nv, uint32_t slices, const Im &im, uint32_t slice, const Rank &rank,
                                        const Add &add) {
    constexpr int E = 16 / sizeof(K), G = SS_VPT / E;
    const bool val16 = ss_al16(vrow);
    const uint32_t nch = (nv + (uint32_t)SS_CHUNK - 1u) / (uint32_t)SS_CHUNK;
    for (uint32_t c = slice; c < nch; c += slices) {
        K v[SS_VPT];
        uint32_t n;  // the thread's values inside the row: the first n of its SS_VPT
        if constexpr (STRIPED) {
            const uint32_t i0 = c * (uint32_t)SS_CHUNK + threadIdx.x;
            if (i0 >= nv) continue;
            const uint32_t left = (nv - i0 + (uint32_t)SS_BLOCK - 1u) / (uint32_t)SS_BLOCK;  // >= 1
            n = left < (uint32_t)SS_VPT ? left : (uint32_t)SS_VPT;
#pragma unroll
            for (int k = 0; k < SS_VPT; ++k) {
                const uint32_t i = i0 + (uint32_t)k * SS_BLOCK;
                v[k] = im.ord(i < nv ? vrow[i] : (K)0);
            }
        } else {
            const uint32_t i0 = c * (uint32_t)SS_CHUNK + threadIdx.x * (uint32_t)SS_VPT;
            if (i0 >= nv) continue;
            const uint32_t left = nv - i0;  // >= 1
            n = left < (uint32_t)SS_VPT ? left : (uint32_t)SS_VPT;
            if (val16 && n == (uint32_t)SS_VPT) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    K t[E];
                    ss_unpack(reinterpret_cast<const uint4 *>(vrow + i0)[g], t);
#pragma unroll
                    for (int k = 0; k < E; ++k) v[g * E + k] = t[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < SS_VPT; ++k) v[k] = (uint32_t)k < left ? vrow[i0 + k] : (K)0;
            }
#pragma unroll
            for (int k = 0; k < SS_VPT; ++k) v[k] = im.ord(v[k]);
        }
        uint32_t pos[SS_VPT];
        rank(v, pos);
        bc_emit(pos, n, add);
    }
}

// nb counters in LDS to the row's output
__device__ __forceinline__ void bc_flush(const uint32_t *cnt, uint32_t nb, uint32_t *orow, bool store) {
    for (uint32_t b = threadIdx.x; b < nb; b += SS_BLOCK) {
        const uint32_t c = cnt[b];
        if (store)
            orow[b] = c;
        else if (c)
            atomicAdd(orow + b, c);
    }
}

// n words (4-byte aligned, no more) to zero.  A kernel and not hipMemsetAsync: a captured memset
// node left garbage in the output from the second replay on (tests/test_gpu_bucket_counts.py's
// graph test found it; launch_zero of kernels.hip exists for the same reason but wants 16-byte
// alignment).
constexpr int BC_ZERO_BLOCK = 256;
__global__ __launch_bounds__(BC_ZERO_BLOCK) void k_bc_zero(uint32_t *p, size_t n) {
    const size_t stride = (size_t)gridDim.x * BC_ZERO_BLOCK;
    for (size_t i = (size_t)blockIdx.x * BC_ZERO_BLOCK + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

// ---- LDS path: nedges <= bc_row_edges(sizeof(K)); nedges == 0 makes no probe and counts into bin 0
template <class K, class Im>
__global__ __launch_bounds__(SS_BLOCK) void k_bc_lds(BcArgs<K, Im> a) {
    constexpr int E = 16 / sizeof(K);
    constexpr uint32_t EMAX = bc_row_edges(sizeof(K));
    __shared__ __attribute__((aligned(16))) K img[EMAX];
    __shared__ uint32_t cnt[EMAX + 1];
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.slices, slice = blockIdx.x - row * a.slices;
    const uint32_t nb = a.nedges + 1u;
    const K *seq = a.edges + (a.per_row ? (size_t)row * a.nedges : 0);
    if (ss_al16(seq)) {  // (k_ss_lds's staging, without a sorter)
        const uint32_t groups = a.nedges / (uint32_t)E;
        for (uint32_t g = tid; g < groups; g += SS_BLOCK) {
            K t[E];
            ss_unpack(reinterpret_cast<const uint4 *>(seq)[g], t);
#pragma unroll
            for (int k = 0; k < E; ++k) t[k] = a.im.ord(t[k]);
            reinterpret_cast<uint4 *>(img)[g] = ss_pack(t);
        }
        for (uint32_t i = groups * (uint32_t)E + tid; i < a.nedges; i += SS_BLOCK) img[i] = a.im.ord(seq[i]);
    } else {
        for (uint32_t i = tid; i < a.nedges; i += SS_BLOCK) img[i] = a.im.ord(seq[i]);
    }
    for (uint32_t b = tid; b < nb; b += SS_BLOCK) cnt[b] = 0u;
    __syncthreads();
    const SsLdsSeq<K> q = {img, a.nedges};
    const uint32_t top = ss_top(a.nedges);
    const bool right = a.right != 0u;
    bc_walk<false>(
        a.vals + (size_t)row * a.nv, a.nv, a.slices, a.im, slice,
        [&](const K(&v)[SS_VPT], uint32_t(&pos)[SS_VPT]) { ss_rank8<false>(q, top, v, right, pos); },
        [&](uint32_t b, uint32_t c) { atomicAdd(&cnt[b], c); });  // (b <= nedges: ss_rank8's pos <= len)
    __syncthreads();
    bc_flush(cnt, nb, a.out + (size_t)row * nb, a.store != 0u);
}

// ---- long path: k_ss_long's search over k_ss_sample's table, every rank an atomic add on the
// row's zeroed output
template <class K, class Im>
__global__ __launch_bounds__(SS_BLOCK) void k_bc_long(BcArgs<K, Im> a) {
    constexpr int E = 16 / sizeof(K);
    __shared__ __attribute__((aligned(16))) K img[SS_SAMPLES];
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.slices, slice = blockIdx.x - row * a.slices;
    const K *table = a.table + (a.per_row ? (size_t)row * SS_SAMPLES : 0);  // (16-byte aligned: the workspace's regions)
    for (uint32_t g = tid; g < (uint32_t)(SS_SAMPLES / E); g += SS_BLOCK)
        reinterpret_cast<uint4 *>(img)[g] = reinterpret_cast<const uint4 *>(table)[g];
    __syncthreads();
    const uint32_t stride = ss_stride(a.nedges), ns = ss_strides(a.nedges);  // ns >= 1
    const SsLdsSeq<K> q = {img, ns};
    const uint32_t top1 = ss_top(ns), top2 = ss_top(stride - 1u), cols = a.nedges;
    const bool right = a.right != 0u;
    SsStrideSeq<K, Im> g = {a.edges + (a.per_row ? (size_t)row * cols : 0), nullptr, cols, a.im, {}, {}};
    uint32_t *orow = a.out + (size_t)row * (cols + 1u);
    bc_walk<true>(
        a.vals + (size_t)row * a.nv, a.nv, a.slices, a.im, slice,
        [&](const K(&v)[SS_VPT], uint32_t(&pos)[SS_VPT]) {  // (k_ss_long's)
            uint32_t c[SS_VPT];
            ss_rank8<false>(q, top1, v, right, c);
#pragma unroll
            for (int j = 0; j < SS_VPT; ++j) {
                const uint32_t sj = c[j] < ns ? c[j] : ns - 1u;
                g.start[j] = sj * stride;  // < cols
                const uint32_t seg = cols - g.start[j] < stride ? cols - g.start[j] : stride;  // >= 1
                g.last[j] = seg - 1u;
            }
            ss_rank8<true>(g, top2, v, right, pos);
#pragma unroll
            for (int j = 0; j < SS_VPT; ++j) pos[j] = c[j] >= ns ? cols : g.start[j] + g.last[j] - pos[j];  // <= cols
        },
        [&](uint32_t b, uint32_t c) { atomicAdd(orow + b, c); });
}

// ---- bincount: the words as they are (a negative value is a large unsigned one: past nbins)
struct BcPlain {
    template <class K>
    __device__ __forceinline__ K ord(K x) const {
        return x;
    }
};

template <class K>
struct BinArgs {
    const K *vals;    // rows x nv
    uint32_t *out;    // rows x (nbins + 1) counters
    uint32_t nbins, nv, slices, store;
};

template <class K, bool LDS>
__global__ __launch_bounds__(SS_BLOCK) void k_bincount(BinArgs<K> a) {
    __shared__ uint32_t cnt[LDS ? BIN_ROW_BINS + 1 : 1];
    const uint32_t tid = threadIdx.x, row = blockIdx.x / a.slices, slice = blockIdx.x - row * a.slices;
    const uint32_t nbins = a.nbins, nb = nbins + 1u;
    const auto rank = [&](const K(&v)[SS_VPT], uint32_t(&pos)[SS_VPT]) {
#pragma unroll
        for (int j = 0; j < SS_VPT; ++j) pos[j] = v[j] < (K)nbins ? (uint32_t)v[j] : nbins;
    };
    const K *vrow = a.vals + (size_t)row * a.nv;
    uint32_t *orow = a.out + (size_t)row * nb;
    if constexpr (LDS) {
        for (uint32_t b = tid; b < nb; b += SS_BLOCK) cnt[b] = 0u;
        __syncthreads();
        bc_walk<false>(vrow, a.nv, a.slices, BcPlain{}, slice, rank, [&](uint32_t b, uint32_t c) { atomicAdd(&cnt[b], c); });
        __syncthreads();
        bc_flush(cnt, nb, orow, a.store != 0u);
    } else {
        bc_walk<false>(vrow, a.nv, a.slices, BcPlain{}, slice, rank, [&](uint32_t b, uint32_t c) { atomicAdd(orow + b, c); });
    }
}

inline size_t ss_esz(int kt) { return key_type_is16(kt) ? 2 : key_type_is64(kt) ? 8 : 4; }
inline bool ss_key_type_ok(int kt) { return topk_key_type_ok(kt) || key_type_is64(kt); }
inline size_t ss_row_keys(int kt) { return (size_t)SS_LDS_BYTES / ss_esz(kt); }

template <class K, class Im>
int ss_launch(const void *sorted, size_t seq_rows, size_t cols, const uint32_t *sorter, const void *values, size_t rows, size_t nv,
              int right, const Im &im, uint32_t *out, char *ws, hipStream_t s) {
    TimingScope ts(LABSORT_K_SEGSORT, s);
    const bool per_row = seq_rows != 1, lng = cols > SS_LDS_BYTES / sizeof(K);
    // one shared sequence: every value is one row's
    const size_t r = per_row ? rows : 1, n = per_row ? nv : rows * nv;
    SsArgs<K, Im> a = {};
    a.seq = static_cast<const K *>(sorted);
    a.sorter = sorter;
    a.vals = static_cast<const K *>(values);
    a.out = out;
    a.cols = (uint32_t)cols;
    a.nv = (uint32_t)n;
    a.per_row = per_row ? 1u : 0u;
    a.right = right ? 1u : 0u;
    a.im = im;
    // a few workgroups per CU in all, each striding over its row's chunks; at least one per row
    const size_t nch = (n + SS_CHUNK - 1) / SS_CHUNK, cap = (size_t)cu_count() * (lng ? SS_LONG_WG_PER_CU : SS_LDS_WG_PER_CU);
    a.slices = (uint32_t)std::min(nch, std::max<size_t>(1, (cap + r - 1) / r));
    const unsigned grid = (unsigned)(r * a.slices);  // r alone where r >= cap, below 2 cap otherwise
    if (lng) {
        a.hdr = reinterpret_cast<uint32_t *>(ws);
        a.table = reinterpret_cast<K *>(ws + SEG_HDR_BYTES);
        k_ss_sample<K, Im><<<(unsigned)(seq_rows * (SS_SAMPLES / SS_SAMPLE_BLOCK)), SS_SAMPLE_BLOCK, 0, s>>>(a);
        k_ss_long<K, Im><<<grid, SS_BLOCK, 0, s>>>(a);
    } else {
        k_ss_lds<K, Im><<<grid, SS_BLOCK, 0, s>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return LABSORT_OK;
}

// ---- counting: the grid is ss_launch's (row, slice) form, the counts being per row of the values
// whether the edges are shared or not: workgroups per row, a few per CU in all, one per row at least
inline uint32_t bc_slices(size_t rows, size_t nv, int wg_per_cu) {
    const size_t nch = (nv + SS_CHUNK - 1) / SS_CHUNK, cap = (size_t)cu_count() * wg_per_cu;  // nv >= 1
    return (uint32_t)std::min(nch, std::max<size_t>(1, (cap + rows - 1) / rows));
}

inline void bc_zero(uint32_t *out, size_t nwords, hipStream_t s) {
    const size_t blocks = (nwords + BC_ZERO_BLOCK * 4 - 1) / (BC_ZERO_BLOCK * 4);
    k_bc_zero<<<(unsigned)std::min<size_t>(std::max<size_t>(blocks, 1), 2048), BC_ZERO_BLOCK, 0, s>>>(out, nwords);
}

inline size_t bc_row_edges_kt(int kt) { return bc_row_edges(ss_esz(kt)); }
inline size_t bc_ws_bytes(size_t edge_rows, size_t nedges, int kt) {
    return nedges <= bc_row_edges_kt(kt) ? 0 : SEG_HDR_BYTES + edge_rows * ((size_t)SS_SAMPLES * ss_esz(kt));
}

template <class K, class Im>
int bc_launch(const void *edges, size_t edge_rows, size_t nedges, const void *values, size_t rows, size_t nv, int right, const Im &im,
              uint32_t *out, char *ws, hipStream_t s) {
    TimingScope ts(LABSORT_K_SEGSORT, s);
    const bool lng = nedges > bc_row_edges(sizeof(K));
    const uint32_t slices = bc_slices(rows, nv, lng ? SS_LONG_WG_PER_CU : SS_LDS_WG_PER_CU);
    const unsigned grid = (unsigned)(rows * slices);  // rows alone where they fill the CUs, below twice that otherwise
    BcArgs<K, Im> a = {};
    a.edges = static_cast<const K *>(edges);
    a.vals = static_cast<const K *>(values);
    a.out = out;
    a.nedges = (uint32_t)nedges;
    a.nv = (uint32_t)nv;
    a.slices = slices;
    a.per_row = edge_rows != 1 ? 1u : 0u;
    a.right = right ? 1u : 0u;
    a.store = !lng && slices == 1u ? 1u : 0u;
    a.im = im;
    if (!a.store) bc_zero(out, rows * (nedges + 1), s);
    if (lng) {
        SsArgs<K, Im> sa = {};  // k_ss_sample as searchsorted runs it: the header's status word and the tables
        sa.seq = a.edges;
        sa.cols = a.nedges;
        sa.hdr = reinterpret_cast<uint32_t *>(ws);
        sa.table = reinterpret_cast<K *>(ws + SEG_HDR_BYTES);
        sa.im = im;
        a.table = sa.table;
        k_ss_sample<K, Im><<<(unsigned)(edge_rows * (SS_SAMPLES / SS_SAMPLE_BLOCK)), SS_SAMPLE_BLOCK, 0, s>>>(sa);
        k_bc_long<K, Im><<<grid, SS_BLOCK, 0, s>>>(a);
    } else {
        k_bc_lds<K, Im><<<grid, SS_BLOCK, 0, s>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return LABSORT_OK;
}

template <class K>
int bin_launch(const void *values, size_t rows, size_t nv, size_t nbins, uint32_t *out, hipStream_t s) {
    TimingScope ts(LABSORT_K_SEGSORT, s);
    const bool lds = nbins <= (size_t)BIN_ROW_BINS;
    const uint32_t slices = bc_slices(rows, nv, lds ? SS_LDS_WG_PER_CU : SS_LONG_WG_PER_CU);
    const unsigned grid = (unsigned)(rows * slices);
    BinArgs<K> a = {static_cast<const K *>(values), out, (uint32_t)nbins, (uint32_t)nv, slices, lds && slices == 1u ? 1u : 0u};
    if (!a.store) bc_zero(out, rows * (nbins + 1), s);
    if (lds)
        k_bincount<K, true><<<grid, SS_BLOCK, 0, s>>>(a);
    else
        k_bincount<K, false><<<grid, SS_BLOCK, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return LABSORT_OK;
}

}  // namespace

}  // namespace labsort

using namespace labsort;

extern "C" {

size_t labsort_searchsorted_row_keys(int key_type) { return ss_key_type_ok(key_type) ? ss_row_keys(key_type) : 0; }

size_t labsort_searchsorted_chunk_values(void) { return (size_t)SS_CHUNK; }

// header | one table of SS_SAMPLES images per sequence (a multiple of 256 bytes each)
size_t labsort_searchsorted_workspace_bytes(size_t seq_rows, size_t cols, int key_type) {
    static_assert(SS_SAMPLES * 2 % 256 == 0, "the tables lie one behind the other, each 256-byte aligned");
    if (!ss_key_type_ok(key_type) || cols <= ss_row_keys(key_type)) return 0;
    return SEG_HDR_BYTES + seq_rows * ((size_t)SS_SAMPLES * ss_esz(key_type));
}

int labsort_searchsorted_device(const void *d_sorted, size_t seq_rows, size_t cols, const uint32_t *d_sorter, const void *d_values,
                                size_t rows, size_t nv, int right, int key_type, uint32_t *d_out, void *d_ws, size_t ws_bytes,
                                void *stream) {
    if (rows == 0 || nv == 0) return LABSORT_OK;
    if (!ss_key_type_ok(key_type)) return LABSORT_ERR_ARG;
    if (!d_values || !d_out || (cols != 0 && !d_sorted)) return LABSORT_ERR_ARG;
    if (seq_rows != 1 && seq_rows != rows) return LABSORT_ERR_ARG;
    const size_t esz = ss_esz(key_type), lim = 0x7FFFFFFFu;
    if ((((uintptr_t)d_sorted | (uintptr_t)d_values) & (esz - 1)) || (((uintptr_t)d_out | (uintptr_t)d_sorter) & 3u))
        return LABSORT_ERR_ARG;
    if (rows > lim / nv || (cols != 0 && seq_rows > lim / cols)) return LABSORT_ERR_ARG;
    // the output shares no byte with an input
    const size_t nseq = seq_rows * cols, nval = rows * nv;
    if (ranges_overlap(d_out, nval * 4, d_values, nval * esz) || (nseq && ranges_overlap(d_out, nval * 4, d_sorted, nseq * esz)) ||
        (nseq && d_sorter && ranges_overlap(d_out, nval * 4, d_sorter, nseq * 4)))
        return LABSORT_ERR_ARG;
    const size_t need = labsort_searchsorted_workspace_bytes(seq_rows, cols, key_type);
    if (need && (!d_ws || ws_bytes < need || ((uintptr_t)d_ws & 15u) || ranges_overlap(d_out, nval * 4, d_ws, need)))
        return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    if (cols == 0) {
        HIP_TRY(hipMemsetAsync(d_out, 0, nval * 4, s));
        return LABSORT_OK;
    }
    char *ws = static_cast<char *>(d_ws);
    if (key_type_is16(key_type))
        return ss_launch<uint16_t>(d_sorted, seq_rows, cols, d_sorter, d_values, rows, nv, right, SsImage16{nan_t16(key_type)}, d_out,
                                   ws, s);
    if (key_type_is64(key_type))
        return ss_launch<uint64_t>(d_sorted, seq_rows, cols, d_sorter, d_values, rows, nv, right, UqImage<uint64_t>{key_type}, d_out,
                                   ws, s);
    return ss_launch<uint32_t>(d_sorted, seq_rows, cols, d_sorter, d_values, rows, nv, right, UqImage<uint32_t>{key_type}, d_out, ws,
                               s);
}

size_t labsort_bucket_counts_row_edges(int key_type) { return ss_key_type_ok(key_type) ? bc_row_edges_kt(key_type) : 0; }

// header | one table of SS_SAMPLES images per edge row, as searchsorted's
size_t labsort_bucket_counts_workspace_bytes(size_t edge_rows, size_t nedges, int key_type) {
    return ss_key_type_ok(key_type) ? bc_ws_bytes(edge_rows, nedges, key_type) : 0;
}

int labsort_bucket_counts_device(const void *d_edges, size_t edge_rows, size_t nedges, const void *d_values, size_t rows, size_t nv,
                                 int right, int key_type, uint32_t *d_counts_out, void *d_ws, size_t ws_bytes, void *stream) {
    if (rows == 0) return LABSORT_OK;
    if (!ss_key_type_ok(key_type)) return LABSORT_ERR_ARG;
    if (!d_counts_out || (nv != 0 && !d_values) || (nedges != 0 && !d_edges)) return LABSORT_ERR_ARG;
    if (edge_rows != 1 && edge_rows != rows) return LABSORT_ERR_ARG;
    const size_t esz = ss_esz(key_type), lim = 0x7FFFFFFFu;
    if ((((uintptr_t)d_edges | (uintptr_t)d_values) & (esz - 1)) || ((uintptr_t)d_counts_out & 3u)) return LABSORT_ERR_ARG;
    if ((nv != 0 && rows > lim / nv) || nedges >= lim || edge_rows > lim / std::max<size_t>(nedges, 1) || rows > lim / (nedges + 1))
        return LABSORT_ERR_ARG;
    // the output shares no byte with an input or the workspace
    const size_t nseq = edge_rows * nedges, nval = rows * nv, ob = rows * (nedges + 1) * 4;
    if ((nval && ranges_overlap(d_counts_out, ob, d_values, nval * esz)) || (nseq && ranges_overlap(d_counts_out, ob, d_edges, nseq * esz)))
        return LABSORT_ERR_ARG;
    const size_t need = bc_ws_bytes(edge_rows, nedges, key_type);
    if (need && (!d_ws || ws_bytes < need || ((uintptr_t)d_ws & 15u) || ranges_overlap(d_counts_out, ob, d_ws, need)))
        return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    if (nv == 0) {
        TimingScope ts(LABSORT_K_SEGSORT, s);
        bc_zero(d_counts_out, ob / 4, s);
        HIP_TRY(hipGetLastError());
        return LABSORT_OK;
    }
    char *ws = static_cast<char *>(d_ws);
    if (key_type_is16(key_type))
        return bc_launch<uint16_t>(d_edges, edge_rows, nedges, d_values, rows, nv, right, SsImage16{nan_t16(key_type)}, d_counts_out, ws,
                                   s);
    if (key_type_is64(key_type))
        return bc_launch<uint64_t>(d_edges, edge_rows, nedges, d_values, rows, nv, right, UqImage<uint64_t>{key_type}, d_counts_out, ws,
                                   s);
    return bc_launch<uint32_t>(d_edges, edge_rows, nedges, d_values, rows, nv, right, UqImage<uint32_t>{key_type}, d_counts_out, ws, s);
}

size_t labsort_bincount_row_bins(void) { return (size_t)BIN_ROW_BINS; }

int labsort_bincount_device(const void *d_values, size_t rows, size_t nv, size_t nbins, int key_type, uint32_t *d_counts_out,
                            void *stream) {
    if (rows == 0) return LABSORT_OK;
    const bool k64 = key_type == LABSORT_KEY_U64 || key_type == LABSORT_KEY_I64;
    if (!k64 && !key_type_ok(key_type)) return LABSORT_ERR_ARG;
    if (!d_counts_out || (nv != 0 && !d_values)) return LABSORT_ERR_ARG;
    const size_t esz = k64 ? 8 : 4, lim = 0x7FFFFFFFu;
    if (((uintptr_t)d_values & (esz - 1)) || ((uintptr_t)d_counts_out & 3u)) return LABSORT_ERR_ARG;
    if ((nv != 0 && rows > lim / nv) || nbins >= lim || rows > lim / (nbins + 1)) return LABSORT_ERR_ARG;
    const size_t nval = rows * nv, ob = rows * (nbins + 1) * 4;
    if (nval && ranges_overlap(d_counts_out, ob, d_values, nval * esz)) return LABSORT_ERR_ARG;
    hipStream_t s = as_stream(stream);
    if (nv == 0) {
        TimingScope ts(LABSORT_K_SEGSORT, s);
        bc_zero(d_counts_out, ob / 4, s);
        HIP_TRY(hipGetLastError());
        return LABSORT_OK;
    }
    return k64 ? bin_launch<uint64_t>(d_values, rows, nv, nbins, d_counts_out, s)
               : bin_launch<uint32_t>(d_values, rows, nv, nbins, d_counts_out, s);
}

}  // extern "C"
