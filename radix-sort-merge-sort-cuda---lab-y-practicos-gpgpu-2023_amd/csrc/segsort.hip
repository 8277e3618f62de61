// segsort.hip -- segmented sort: many independent [start, end) ranges of one buffer sorted
// in one call (labsort_sort_segments_device / labsort_sort_segments_pairs_device).
//
//   k_seg_bin    one thread per segment: validates the offsets and appends the segment to
//                the list of its length class (wave-aggregated, one global atomic per
//                workgroup and class)
//   k_seg_wave   the three wave classes: one wave64 per segment, wave-private LDS, no workgroup
//                barrier; up to 64 keys by counting ranks in registers, longer ones by 8-bit
//                LSD passes (4, 8 or 16 keys per lane)
//   k_seg_block  block and tile classes: k_tile_sort's LDS passes on a [start, end) range,
//                one workgroup per segment, grid-stride over the class list
//   k_fin_edges  the hybrid radix sort's finish: the bucket offsets, from the digit-3 pass's look-back words
//   k_fin_block  (fin_block.h) the block class of the hybrid radix sort's finish
//   k_seg_ids, k_seg_gather, k_seg_err_acc   the general path's glue around the pair sorts
// k_seg_wave and k_seg_block live in seg_kernels.h: this file compiles their integer-key
// instantiations, segsort_f32.hip the float32 ones.
//
// Every kernel after k_seg_bin reads the workspace's error word first and returns when
// it is set, so rejected offsets never become addresses.
#include "segsort.h"

#include <algorithm>

#include "devutil.h"
#include "fin_block.h"
#include "host.h"
#include "seg_kernels.h"

namespace labsort {

namespace {

constexpr int BIN_BLOCK = 1024, BIN_SPT = 4;  // 4096 segments per workgroup

__global__ __launch_bounds__(BIN_BLOCK) void k_seg_bin(const uint32_t *__restrict__ off, uint32_t nseg, uint32_t n,
                                                        uint32_t max_len, SegEdges e, uint32_t copy1,
                                                        uint32_t *__restrict__ hdr, uint32_t *__restrict__ lists,
                                                        size_t stride, const Plan *__restrict__ hyplan) {
    __shared__ uint32_t cnt[SEG_CLASSES], base[SEG_CLASSES];
    if (hyplan && hyplan->hybrid == 0u) return;  // the radix sort's finish, classic path chosen: no offsets
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < (uint32_t)SEG_CLASSES) cnt[tid] = 0u;
    __syncthreads();
    uint32_t cls[BIN_SPT], pos[BIN_SPT];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < BIN_SPT; ++j) {
        const uint32_t seg = blockIdx.x * (uint32_t)(BIN_BLOCK * BIN_SPT) + (uint32_t)j * BIN_BLOCK + tid;
        uint32_t c = SEG_CLASSES;  // none: nothing to sort or copy
        if (seg < nseg) {
            const uint32_t a = off[seg], b = off[seg + 1];
            if (b < a || b > n) {
                bad = true;
            } else {
                const uint32_t len = b - a;
                if (max_len && len > max_len) bad = true;
                if (len > 1u || (len == 1u && copy1)) {
                    c = 0u;
#pragma unroll
                    for (int q = 0; q < SEG_CLASSES - 1; ++q) c += len > e.e[q] ? 1u : 0u;
                }
            }
            if (seg == 0u && a != 0u) bad = true;
            if (seg == nseg - 1u && b != n) bad = true;
        }
        cls[j] = c;
        pos[j] = 0u;
        if (lists) {
#pragma unroll
            for (uint32_t cc = 0; cc < (uint32_t)SEG_CLASSES; ++cc) {
                const uint64_t m = __ballot(c == cc);
                if (m == 0ull) continue;  // wave-uniform
                const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
                uint32_t wb = 0u;
                if (lane == leader) wb = atomicAdd(&cnt[cc], (uint32_t)__popcll(m));
                wb = __shfl(wb, (int)leader);
                if (c == cc) pos[j] = wb + mbcnt64(m);
            }
        }
    }
    if (bad) atomicOr(hdr, 1u);
    if (!lists) return;
    __syncthreads();
    if (tid < (uint32_t)SEG_CLASSES) base[tid] = cnt[tid] ? atomicAdd(hdr + SEG_HDR_CNT + tid, cnt[tid]) : 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BIN_SPT; ++j) {
        const uint32_t seg = blockIdx.x * (uint32_t)(BIN_BLOCK * BIN_SPT) + (uint32_t)j * BIN_BLOCK + tid;
        // (a class list holds at most nseg entries: one per segment)
        if (cls[j] < (uint32_t)SEG_CLASSES) lists[(size_t)cls[j] * stride + base[cls[j]] + pos[j]] = seg;
    }
}

// ---------------------------------------------------------------------------------
// general path glue
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_ids(const uint32_t *__restrict__ off, uint32_t nseg, uint32_t n,
                                                 const uint32_t *__restrict__ idx, uint32_t *__restrict__ ids,
                                                 uint32_t *__restrict__ iota, const uint32_t *__restrict__ hdr) {
    if (ld_agent(hdr) != 0u) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (iota) iota[i] = (uint32_t)i;
        if (!ids) continue;
        uint32_t p = idx ? idx[i] : (uint32_t)i;
        if (p >= n) p = n - 1u;
        // first q in [1, nseg] with off[q] > p (off[nseg] = n > p): p lies in segment q - 1
        uint32_t lo = 1u, hi = nseg;
        while (lo < hi) {  // first position in [lo, hi) with (key ^ flip) >> 16 >= q
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (off[mid] > p) hi = mid;
            else lo = mid + 1u;
        }
        ids[i] = lo - 1u;
    }
}

__global__ __launch_bounds__(256) void k_seg_gather(const uint32_t *__restrict__ src, const uint32_t *__restrict__ vsrc,
                                                    const uint32_t *__restrict__ perm, uint32_t *__restrict__ out,
                                                    uint32_t *__restrict__ vout, uint32_t n,
                                                    const uint32_t *__restrict__ hdr) {
    if (ld_agent(hdr) != 0u) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t p = perm ? perm[i] : (uint32_t)i;
        if (p >= n) p = n - 1u;
        out[i] = src[p];
        if (vsrc) vout[i] = vsrc[p];
    }
}

__global__ void k_seg_err_acc(uint32_t *hdr, uint32_t *inner) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (*inner) hdr[SEG_HDR_DEVERR] = 1u;
        *inner = 0u;
    }
}

unsigned stream_blocks(size_t n) {
    size_t b = (n + 256 * 8 - 1) / (256 * 8);
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

// The sort kernel of class c (0-2 wave, 3 block, 4 tile) over its list; vin/vout nullptr: keys only.
hipError_t launch_seg_sort(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                           const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                           hipStream_t s, const HySel &hy = HySel{}, bool f32 = false) {
    return f32 ? launch_seg_sort_f32(c, in, out, vin, vout, off, hdr, list, flip, s, hy)
               : launch_seg_sort_t<false>(c, in, out, vin, vout, off, hdr, list, flip, s, hy);
}

// general path helpers (all return at once when hdr word 0 is set)
// ids[i] = segment of position (idx ? idx[i] : i); iota (or nullptr): iota[i] = i
hipError_t launch_seg_ids(const uint32_t *off, size_t nseg, size_t n, const uint32_t *idx, uint32_t *ids,
                          uint32_t *iota, const uint32_t *hdr, hipStream_t s) {
    k_seg_ids<<<stream_blocks(n), 256, 0, s>>>(off, (uint32_t)nseg, (uint32_t)n, idx, ids, iota, hdr);
    return hipGetLastError();
}

// out[i] = perm ? src[perm[i]] : src[i], for keys and (vsrc != nullptr) payloads
hipError_t launch_seg_gather(const uint32_t *src, const uint32_t *vsrc, const uint32_t *perm, uint32_t *out,
                             uint32_t *vout, size_t n, const uint32_t *hdr, hipStream_t s) {
    k_seg_gather<<<stream_blocks(n), 256, 0, s>>>(src, vsrc, perm, out, vout, (uint32_t)n, hdr);
    return hipGetLastError();
}

// hdr[SEG_HDR_DEVERR] |= *inner_err; *inner_err = 0
hipError_t launch_seg_err_acc(uint32_t *hdr, uint32_t *inner_err, hipStream_t s) {
    k_seg_err_acc<<<1, 64, 0, s>>>(hdr, inner_err);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_seg_bin(const uint32_t *off, size_t nseg, size_t n, size_t max_len, bool pairs, bool copy1,
                          uint32_t *hdr, uint32_t *lists, size_t stride, hipStream_t s) {
    const unsigned g = (unsigned)((nseg + BIN_BLOCK * BIN_SPT - 1) / (BIN_BLOCK * BIN_SPT));
    (void)pairs;  // the class edges below the tile are the same for keys and pairs
    const SegEdges e{{(uint32_t)SEG_WAVE_KEYS, (uint32_t)SEG_WAVE2_KEYS, (uint32_t)SEG_WAVE3_KEYS, (uint32_t)SEG_BLOCK_KEYS}};
    k_seg_bin<<<g, BIN_BLOCK, 0, s>>>(off, (uint32_t)nseg, (uint32_t)n, (uint32_t)max_len, e, copy1 ? 1u : 0u, hdr, lists,
                                      stride, nullptr);
    return hipGetLastError();
}

hipError_t launch_seg_lds_classes(size_t max_len, bool pairs, const uint32_t *in, uint32_t *out, const uint32_t *vin,
                                  uint32_t *vout, const uint32_t *off, const uint32_t *hdr, const uint32_t *lists,
                                  size_t stride, uint32_t flip, bool f32, hipStream_t s) {
    (void)pairs;  // the class edges below the tile are the same for keys and pairs
    for (int c = 0; c <= seg_class_of(max_len); ++c) {
        const hipError_t e = launch_seg_sort(c, in, out, vin, vout, off, hdr, lists + (size_t)c * stride, flip, s, HySel{}, f32);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------------
// the hybrid radix sort's finish
// ---------------------------------------------------------------------------------
namespace {
constexpr int FE_BLOCK = 1024, FE_W = FE_BLOCK / WAVE, FE_KPT = OSP_TILE / FE_BLOCK;
static_assert(FE_KPT * FE_BLOCK == OSP_TILE && HY_BUCKETS == 256u * 256u, "one tile per boundary, one workgroup per digit-2 value");

// Where the digit-3 pass put, for each digit-3 value d (thread d < 256; the other threads' result
// means nothing), the first key of digit d that lay at or after position P of its input: the
// segment's base, the inclusive prefix the tile before P's tile published in the pass's look-back
// region (every slot holds LB_INC | prefix once the pass is through), and the keys of digit d in
// P's tile before P, counted here.  P's segment is the last one that starts at or before P, its tile
// by k_onesweep_p's tile_range: aligned to OSP_TILE but for a segment's first.  A look-back word
// without LB_INC, or a slot outside the region, sets `bad`.  wh: FE_W * 256 words of LDS.
__device__ uint32_t fin_edge_at(uint32_t P, const uint32_t *__restrict__ keys, uint32_t flip, const SegPlan *__restrict__ sp,
                                const uint32_t *__restrict__ lb, uint32_t nslots, uint32_t *wh, bool &bad) {
    const uint32_t tid = threadIdx.x, wid = tid >> 6;
    uint32_t sg = 0;
    for (uint32_t s = 1; s < (uint32_t)NSEG; ++s) sg = sp->start[s] <= P ? s : sg;  // (the starts ascend)
    const uint32_t s0 = sp->start[sg], a0 = s0 - s0 % (uint32_t)OSP_TILE;
    const uint32_t l = (P - a0) / (uint32_t)OSP_TILE, beg = l ? a0 + l * (uint32_t)OSP_TILE : s0;
    for (uint32_t i = tid; i < (uint32_t)(FE_W * 256); i += FE_BLOCK) wh[i] = 0u;
    uint32_t k[FE_KPT];
#pragma unroll
    for (int j = 0; j < FE_KPT; ++j) {
        const uint32_t i = beg + (uint32_t)j * FE_BLOCK + tid;
        k[j] = i < P ? keys[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FE_KPT; ++j)
        if (beg + (uint32_t)j * FE_BLOCK + tid < P) atomicAdd(&wh[wid * 256u + ((k[j] ^ flip) >> 24)], 1u);
    __syncthreads();
    if (tid >= 256u) return 0u;
    uint32_t r = sp->base[sg * 256u + tid];
#pragma unroll
    for (int w = 0; w < FE_W; ++w) r += wh[(uint32_t)w * 256u + tid];
    if (l) {
        const uint32_t slot = sp->tpre[sg] + l - 1u;
        const uint32_t w = slot < nslots ? lb[(size_t)slot * 256u + tid] : 0u;
        if ((w & LB_INC) == 0u) bad = true;
        r += w & LB_VAL;
    }
    return r;
}

// The finish's bucket offsets, from what the digit-3 pass left behind: off[q] = first position whose
// key's top 16 bits are >= q for the HY_BUCKETS buckets q = (d3 << 8) | d2, and off[HY_BUCKETS] = n.
// The digit-3 pass's input is ordered by digit 2 and the scatter is stable, so bucket (d3, d2) starts
// where the pass put the first key of digit d3 at or after input position S2[d2], the number of keys
// with a smaller digit 2 (fin_edge_at).  One workgroup per d2, thread d3 < 256 writes one offset;
// hist: the four digits' totals as k_plan8 leaves them.  Digit 3 constant (plan->src[3] is SKIP,
// no pass ran, its SegPlan and look-back region are not read): the offsets are 0 below that digit,
// S2[d2] at it and n above, which is the digit-3 totals' exclusive scan, plus S2[d2] at the digit.
// An unfinished look-back word sets both error words, the radix workspace's (err) and the
// finish's (hdr), which every class kernel reads first; no offset is written from it.
// (The workgroup also finding the offsets of d2 + 1 and appending its 256 buckets to the class lists,
// in place of the k_seg_bin launch: 12.6 us against 9.2 + 6.3, but the lists then run in steps of 256
// buckets and k_fin_block took 593 us against 587; harness/exp/fin_edges_fused_bin.patch.)
__global__ __launch_bounds__(FE_BLOCK) void k_fin_edges(const Plan *__restrict__ plan, Bufs bufs, uint32_t n, uint32_t flip,
                                                        const uint32_t *__restrict__ hist, const SegPlan *__restrict__ sp,
                                                        const uint32_t *__restrict__ lb, uint32_t nslots, uint32_t *err,
                                                        uint32_t *hdr, uint32_t *__restrict__ off) {
    __shared__ uint32_t wh[FE_W * 256];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t s2;
    if (plan->hybrid == 0u) return;
    const uint32_t tid = threadIdx.x, d2 = blockIdx.x;
    const uint32_t h2 = tid < 256u ? hist[2 * 256 + tid] : 0u;
    const uint32_t x2 = block_excl_scan<FE_BLOCK, 256>(h2, wsum);
    if (tid == d2) s2 = min(x2, n);
    __syncthreads();
    const uint32_t P = s2;
    uint32_t o;
    bool bad = false;
    if (plan->src[3] == SEL_SKIP) {
        const uint32_t h3 = tid < 256u ? hist[3 * 256 + tid] : 0u;
        o = block_excl_scan<FE_BLOCK, 256>(h3, wsum) + (h3 == n ? P : 0u);
    } else {
        // (the pass's input, which it leaves as it was on every buffer plan)
        o = fin_edge_at(P, bufs.p[plan->src[3]], flip, sp, lb, nslots, wh, bad);
    }
    if (tid >= 256u) return;
    if (bad) {
        atomicOr(err, 1u);
        atomicOr(hdr, 1u);
        return;
    }
    const uint32_t q = (tid << 8) | d2;
    off[q] = o;
    if (q == HY_BUCKETS - 1u) off[HY_BUCKETS] = n;
}
}  // namespace

hipError_t launch_hybrid_finish(const Plan *plan, Bufs b, size_t n, uint32_t flip, const uint32_t *hist, const SegPlan *sp3,
                                const uint32_t *lookback3, size_t nslots, uint32_t *err, uint32_t *hdr, uint32_t *off,
                                uint32_t *lists, hipStream_t s) {
    const size_t stride = HY_BUCKETS;
    k_fin_edges<<<256, FE_BLOCK, 0, s>>>(plan, b, (uint32_t)n, flip, hist, sp3, lookback3, (uint32_t)nslots, err, hdr, off);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // every bucket is written (the finish may read TMP or IN and write OUT): one-key buckets are listed
    const SegEdges ed{{(uint32_t)SEG_WAVE_KEYS, (uint32_t)SEG_WAVE2_KEYS, (uint32_t)SEG_WAVE3_KEYS, (uint32_t)HY_BLOCK_KEYS}};
    k_seg_bin<<<HY_BUCKETS / (BIN_BLOCK * BIN_SPT), BIN_BLOCK, 0, s>>>(off, HY_BUCKETS, (uint32_t)n, HY_MAX_BUCKET, ed, 1u, hdr,
                                                                      lists, stride, plan);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const HySel hy{plan, {b.p[0], b.p[1], b.p[2]}};
    uint32_t *out = b.p[SEL_OUT];
    const unsigned cus = (unsigned)cu_count();
    for (int c = 0; c < SEG_CLASSES; ++c) {
        const uint32_t *list = lists + (size_t)c * stride;
        if (c == 3) {  // the finish's own block class, its list handed out by the header's ticket
            k_fin_block<HY_BLOCK, HY_BLOCK_KPT, HY_BLOCK_WPE><<<cus * (unsigned)HY_BLOCK_WPE, HY_BLOCK, 0, s>>>(
                out, off, hdr, list, hdr + SEG_HDR_TICKET, hy);
            e = hipGetLastError();
        } else {
            e = launch_seg_sort(c, out, out, nullptr, nullptr, off, hdr, list, flip, s, hy);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the inner pair sort runs LABSORT_ALGO_AUTO; sized so the function never shrinks as n grows
// across AUTO's merge -> radix switch
size_t seg_inner_bytes(size_t n) {
    const size_t m = n < (size_t)LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS ? n : (size_t)LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS;
    return std::max(labsort_pairs_workspace_bytes(n, LABSORT_ALGO_AUTO), labsort_pairs_workspace_bytes(m, LABSORT_ALGO_MERGE));
}

}  // namespace labsort

using namespace labsort;

extern "C" {

// ---------------------------------------------------------------------------------
// host driver and C-ABI: segment i = [d_offsets[i], d_offsets[i+1])
// ---------------------------------------------------------------------------------
size_t labsort_segment_tile_keys(void) { return (size_t)SEG_TILE_KEYS; }
size_t labsort_segment_pair_tile_keys(void) { return (size_t)SEG_TILE_PAIRS; }

int labsort_segment_class_edges(int pairs, size_t *edges, int cap) {
    const size_t e[SEG_CLASSES] = {(size_t)SEG_WAVE_KEYS, (size_t)SEG_WAVE2_KEYS, (size_t)SEG_WAVE3_KEYS, (size_t)SEG_BLOCK_KEYS,
                                   pairs ? (size_t)SEG_TILE_PAIRS : (size_t)SEG_TILE_KEYS};
    for (int i = 0; i < SEG_CLASSES && i < cap && edges; ++i) edges[i] = e[i];
    return SEG_CLASSES;
}

namespace {
bool seg_lds_path(size_t max_len, int pairs) {
    return max_len > 0 && max_len <= (pairs ? (size_t)SEG_TILE_PAIRS : (size_t)SEG_TILE_KEYS);
}
// LDS path: header | one list of nseg words per class.
// General path: header | three n-word buffers | the inner pair sorts' workspace.
struct SegLayout {
    size_t off_lists, list_stride;    // LDS path (stride in words)
    size_t off_a, off_b, off_c, off_inner, inner_bytes;  // general path
    size_t total;
};
SegLayout seg_layout(size_t n, size_t nseg, bool lds) {
    SegLayout L{};
    Carver c{SEG_HDR_BYTES};
    if (lds) {
        L.list_stride = align_up(nseg * 4, 256) / 4;
        L.off_lists = c.take((size_t)SEG_CLASSES * L.list_stride * 4);
        L.total = c.o;
    } else {
        L.off_a = c.take(n * 4);
        L.off_b = c.take(n * 4);
        L.off_c = c.take(n * 4);
        L.off_inner = c.o;
        L.inner_bytes = seg_inner_bytes(n);
        L.total = c.o + L.inner_bytes;
    }
    return L;
}

int sort_segments(const uint32_t *ki, const uint32_t *vi, uint32_t *ko, uint32_t *vo, size_t n, const uint32_t *off,
                  size_t nseg, size_t max_len, int key_type, void *d_ws, size_t ws_bytes, void *stream) {
    const bool pairs = vi != nullptr || vo != nullptr;
    if (n == 0) return LABSORT_OK;
    if (!ki || !ko || !off || (pairs && (!vi || !vo))) return LABSORT_ERR_ARG;
    if (!device_key_type_ok(key_type)) return LABSORT_ERR_ARG;
    if (nseg == 0 || n > (size_t)0x7FFFFFFFu || nseg > (size_t)0x7FFFFFFFu) return LABSORT_ERR_ARG;
    if (pairs && !pairs_alias_ok(ki, vi, ko, vo)) return LABSORT_ERR_ARG;
    const bool lds = seg_lds_path(max_len, pairs ? 1 : 0);
    if (!lds && n > RADIX_MAX_N) return LABSORT_ERR_ARG;
    if (!d_ws || ws_bytes < labsort_segments_workspace_bytes(n, nseg, max_len, pairs ? 1 : 0)) return LABSORT_ERR_ARG;
    const SegLayout L = seg_layout(n, nseg, lds);
    const uint32_t flip = flip_of(key_type);
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(d_ws);
    uint32_t *hdr = reinterpret_cast<uint32_t *>(ws);
    const bool inplace = ki == ko;
    HIP_TRY(launch_zero(hdr, SEG_HDR_BYTES, s));  // (a kernel: graph-replayable)
    if (lds) {
        uint32_t *lists = reinterpret_cast<uint32_t *>(ws + L.off_lists);
        TimingScope ts(LABSORT_K_SEGSORT, s);
        HIP_TRY(launch_seg_bin(off, nseg, n, max_len, pairs, !inplace, hdr, lists, L.list_stride, s));
        HIP_TRY(launch_seg_lds_classes(max_len, pairs, ki, ko, vi, vo, off, hdr, lists, L.list_stride, flip,
                                       key_type == LABSORT_KEY_F32, s));
        return LABSORT_OK;
    }
    // general path: two stable pair sorts (by key, then by segment id) on workspace buffers;
    // the caller's output is written by the last, guarded, kernel only
    uint32_t *A = reinterpret_cast<uint32_t *>(ws + L.off_a), *B = reinterpret_cast<uint32_t *>(ws + L.off_b),
             *C = reinterpret_cast<uint32_t *>(ws + L.off_c);
    char *iws = ws + L.off_inner;
    uint32_t *ierr = reinterpret_cast<uint32_t *>(iws);
    HIP_TRY(launch_zero(ierr, 16, s));  // (a one-tile inner sort has no error word of its own)
    {
        TimingScope ts(LABSORT_K_SEGSORT, s);
        HIP_TRY(launch_seg_bin(off, nseg, n, max_len, pairs, false, hdr, nullptr, 0, s));
        if (pairs) HIP_TRY(launch_seg_ids(off, nseg, n, nullptr, nullptr, A, hdr, s));  // A = 0, 1, 2, ...
        else HIP_TRY(launch_seg_ids(off, nseg, n, nullptr, A, nullptr, hdr, s));        // A = segment of each position
    }
    int st;
    // (key, A) by key -> (B, C)
    if ((st = labsort_sort_pairs_device(ki, A, B, C, n, key_type, LABSORT_ALGO_AUTO, iws, L.inner_bytes, stream))) return st;
    HIP_TRY(launch_seg_err_acc(hdr, ierr, s));
    if (pairs) {
        // C = positions in key order; B = their segments; (B, C) by segment in place: C = the permutation
        {
            TimingScope ts(LABSORT_K_SEGSORT, s);
            HIP_TRY(launch_seg_ids(off, nseg, n, C, B, nullptr, hdr, s));
        }
        if ((st = labsort_sort_pairs_device(B, C, B, C, n, LABSORT_KEY_U32, LABSORT_ALGO_AUTO, iws, L.inner_bytes, stream)))
            return st;
        HIP_TRY(launch_seg_err_acc(hdr, ierr, s));
        TimingScope ts(LABSORT_K_SEGSORT, s);
        if (inplace) {  // through temporaries: the gather reads what it would overwrite
            HIP_TRY(launch_seg_gather(ki, vi, C, A, B, n, hdr, s));
            HIP_TRY(launch_seg_gather(A, B, nullptr, ko, vo, n, hdr, s));
        } else {
            HIP_TRY(launch_seg_gather(ki, vi, C, ko, vo, n, hdr, s));
        }
    } else {
        // (C = segment ids, B = keys) by segment id in place: B = the result
        if ((st = labsort_sort_pairs_device(C, B, C, B, n, LABSORT_KEY_U32, LABSORT_ALGO_AUTO, iws, L.inner_bytes, stream)))
            return st;
        HIP_TRY(launch_seg_err_acc(hdr, ierr, s));
        TimingScope ts(LABSORT_K_SEGSORT, s);
        HIP_TRY(launch_seg_gather(B, nullptr, nullptr, ko, nullptr, n, hdr, s));
    }
    return LABSORT_OK;
}
}  // namespace

size_t labsort_segments_workspace_bytes(size_t n, size_t nseg, size_t max_segment_keys, int pairs) {
    return seg_layout(n, nseg, seg_lds_path(max_segment_keys, pairs)).total;
}

int labsort_sort_segments_device(const void *d_keys_in, void *d_keys_out, size_t n, const uint32_t *d_offsets,
                                 size_t nseg, size_t max_segment_keys, int key_type, void *d_ws, size_t ws_bytes,
                                 void *stream) {
    return sort_segments(static_cast<const uint32_t *>(d_keys_in), nullptr, static_cast<uint32_t *>(d_keys_out), nullptr,
                         n, d_offsets, nseg, max_segment_keys, key_type, d_ws, ws_bytes, stream);
}

int labsort_sort_segments_pairs_device(const void *d_keys_in, const void *d_vals_in, void *d_keys_out, void *d_vals_out,
                                       size_t n, const uint32_t *d_offsets, size_t nseg, size_t max_segment_keys,
                                       int key_type, void *d_ws, size_t ws_bytes, void *stream) {
    if (n == 0) return LABSORT_OK;
    if (!d_vals_in || !d_vals_out) return LABSORT_ERR_ARG;
    return sort_segments(static_cast<const uint32_t *>(d_keys_in), static_cast<const uint32_t *>(d_vals_in),
                         static_cast<uint32_t *>(d_keys_out), static_cast<uint32_t *>(d_vals_out), n, d_offsets, nseg,
                         max_segment_keys, key_type, d_ws, ws_bytes, stream);
}

int labsort_segments_workspace_status(const void *d_ws, void *stream) {
    uint32_t w[2] = {0, 0};
    if (const int st = read_ws_words(d_ws, w, 2, as_stream(stream))) return st;
    return w[0] ? LABSORT_ERR_ARG : w[SEG_HDR_DEVERR] ? LABSORT_ERR_DEVICE : LABSORT_OK;
}

}  // extern "C"
