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
//   k_seg_ids, k_seg_gather, k_seg_err_acc   the general path's glue around the pair sorts
//
// Every kernel after k_seg_bin reads the workspace's error word first and returns when
// it is set, so rejected offsets never become addresses.
#include "segsort.h"

#include <algorithm>

#include "devutil.h"
#include "lds_pass.h"
#include "host.h"

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
// wave class
// ---------------------------------------------------------------------------------
template <int KPT, bool KV>
struct SwSmem {
    uint32_t keys[WAVE * KPT];
    uint32_t vals[KV ? WAVE * KPT : 1];
    uint32_t hist[256];
    uint32_t probe[WAVE];
};

template <int KPT, bool KV>
__global__ __launch_bounds__(SEG_WAVE_WPB * WAVE) void k_seg_wave(const uint32_t *in, uint32_t *out, const uint32_t *vin,
                                                                  uint32_t *vout, const uint32_t *__restrict__ off,
                                                                  const uint32_t *__restrict__ hdr,
                                                                  const uint32_t *__restrict__ list, int cls,
                                                                  uint32_t flip, HySel hy) {
    constexpr uint32_t CAP = WAVE * KPT;
    __shared__ SwSmem<KPT, KV> sm_all[SEG_WAVE_WPB];
    if (hy.plan) {  // the radix sort's finish: the plan's choice first, and the buffer it names
        if (hy.plan->hybrid == 0u) return;
        in = hy.buf[hy.plan->fin_src];
    }
    if (ld_agent(hdr) != 0u) return;  // rejected offsets: touch nothing
    const uint32_t cnt = hdr[SEG_HDR_CNT + cls];
    const uint32_t lane = threadIdx.x & 63u, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x * SEG_WAVE_WPB + wid >= cnt) return;  // (an empty class costs its launch only)
    SwSmem<KPT, KV> &sm = sm_all[wid];
    const uint32_t sentinel = ~flip;
    const bool atomic_rank = lds_lane_ordered(sm.probe, lane);
    for (uint32_t it = blockIdx.x * SEG_WAVE_WPB + wid; it < cnt; it += gridDim.x * SEG_WAVE_WPB) {
        const uint32_t seg = __builtin_amdgcn_readfirstlane(list[it]);
        const uint32_t b = __builtin_amdgcn_readfirstlane(off[seg]);
        const uint32_t len = __builtin_amdgcn_readfirstlane(off[seg + 1]) - b;
        if (len == 0u || len > CAP) continue;
        if (len <= (uint32_t)WAVE) {
            // one key per lane: its stable rank is the count of keys before it in (key, lane) order
            const bool ok = lane < len;
            const uint32_t x = ok ? (in[b + lane] ^ flip) : 0xFFFFFFFFu;
            uint32_t v = 0u;
            if constexpr (KV) v = ok ? vin[b + lane] : 0u;
            uint32_t r = 0u;
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t xi = __builtin_amdgcn_readlane(x, (int)i);
                r += (xi < x || (xi == x && i < lane)) ? 1u : 0u;
            }
            if (ok) {  // r < len: fewer than len keys come before one of them
                out[b + r] = x ^ flip;
                if constexpr (KV) vout[b + r] = v;
            }
            continue;
        }
        const uint32_t jn = (len + WAVE - 1u) / WAVE;  // 64-key groups that hold keys (<= KPT)
        uint32_t k[KPT];
        uint32_t v[KV ? KPT : 1];
        uint32_t a = ~0u, o = 0u;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t idx = (uint32_t)j * WAVE + lane;
            const bool ok = idx < len;
            k[j] = ok ? in[b + idx] : sentinel;
            if constexpr (KV) v[j] = ok ? vin[b + idx] : 0u;
            const uint32_t x = k[j] ^ flip;
            a &= ok ? x : ~0u;
            o |= ok ? x : 0u;
        }
        wave_and_or(a, o);
        const uint32_t diff = __builtin_amdgcn_readfirstlane(a ^ o);
        for (int pass = 0; pass < 4; ++pass) {
            const uint32_t shift = pass * 8;
            if (((diff >> shift) & 0xFFu) == 0u) continue;  // uniform over the segment
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
                uint32_t xs = s;
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
            if (idx < len) {
                out[b + idx] = k[j];
                if constexpr (KV) vout[b + idx] = v[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// block and tile classes: the passes k_tile_sort runs (lds_sort_passes, lds_pass.h) on one
// segment per workgroup.  The segment is striped over the waves in runs of
// S = 64 ceil(len / (64 W)) slots, so a short segment of the class costs every wave the same
// few 64-key groups; groups that start past the end are neither ranked nor read back
// (LeadingGroups).
// ---------------------------------------------------------------------------------
template <int BLOCK, int KPT, bool KV, int WPE = 4>
__global__ __launch_bounds__(BLOCK, WPE) void k_seg_block(const uint32_t *in, uint32_t *out, const uint32_t *vin,
                                                           uint32_t *vout, const uint32_t *__restrict__ off,
                                                           const uint32_t *__restrict__ hdr,
                                                           const uint32_t *__restrict__ list, int cls, uint32_t flip,
                                                           HySel hy) {
    using S = TsSmem<BLOCK, KPT, KV>;
    constexpr int W = S::W;
    constexpr uint32_t TILE = S::TILE;
    __shared__ S sm;
    if (hy.plan) {  // the radix sort's finish: the plan's choice first, and the buffer it names
        if (hy.plan->hybrid == 0u) return;
        in = hy.buf[hy.plan->fin_src];
    }
    if (ld_agent(hdr) != 0u) return;  // rejected offsets: touch nothing
    const uint32_t cnt = hdr[SEG_HDR_CNT + cls];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t sentinel = ~flip;
    if (blockIdx.x >= cnt) return;  // (an empty class costs its launch only; uniform over the workgroup)
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    __syncthreads();
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    // the list entry and the two offsets are three dependent loads: those of the next segment
    // are issued before this one is sorted
    uint32_t nb = 0u, ne = 0u;
    if (blockIdx.x < cnt) {
        const uint32_t seg = __builtin_amdgcn_readfirstlane(list[blockIdx.x]);
        nb = __builtin_amdgcn_readfirstlane(off[seg]);
        ne = __builtin_amdgcn_readfirstlane(off[seg + 1]);
    }
    for (uint32_t it = blockIdx.x; it < cnt; it += gridDim.x) {
        const uint32_t b = nb, len = ne - nb;
        if (it + gridDim.x < cnt) {
            const uint32_t seg = __builtin_amdgcn_readfirstlane(list[it + gridDim.x]);
            nb = __builtin_amdgcn_readfirstlane(off[seg]);
            ne = __builtin_amdgcn_readfirstlane(off[seg + 1]);
        }
        if (len == 0u || len > TILE) continue;  // (uniform over the workgroup)
        const uint32_t jn = (len + (uint32_t)(W * WAVE) - 1u) / (uint32_t)(W * WAVE);  // groups per wave, <= KPT
        const uint32_t ws0 = wid * jn * WAVE;  // first slot of this wave's stripe
        // this wave's keys: nf whole 64-key groups and a last group of `tail` keys (wave-uniform),
        // so whole groups load and store under scalar branches and one lane mask serves the last
        const uint32_t rem = ws0 < len ? len - ws0 : 0u;
        const uint32_t nf = min(jn, rem / WAVE);
        const uint32_t tail = nf < jn ? rem - nf * WAVE : 0u;  // < 64
        const uint32_t ng = nf + (tail ? 1u : 0u);             // groups that hold keys
        const bool tail_ok = lane < tail;
        // scalar base + 32-bit lane offset per access: the lane offsets pass through empty asms so no
        // 64-bit per-lane address of in / out is formed outside the segment loop and held across it
        const size_t sb = (size_t)b + ws0;
        uint32_t lin = lane;
        asm volatile("" : "+v"(lin));
        uint32_t k[KPT];
        uint32_t v[KV ? KPT : 1];
        uint32_t a = ~0u, o = 0u;
        // every load first, so all of them are in flight together (a use inside the scalar
        // branches would wait for each load in turn), then the bits the keys differ in
        if (nf == (uint32_t)KPT) {  // a whole tile: straight-line loads, as k_tile_sort
#pragma unroll
            for (int j = 0; j < KPT; ++j) k[j] = ld_stream<NT_TILE>(in + sb + ((uint32_t)(j * WAVE) + lin));
            if constexpr (KV) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) v[j] = vin[sb + ((uint32_t)(j * WAVE) + lin)];
            }
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                k[j] = sentinel;
                if constexpr (KV) v[j] = 0u;
                if ((uint32_t)j < nf || ((uint32_t)j == nf && tail_ok)) {
                    k[j] = ld_stream<NT_TILE>(in + sb + ((uint32_t)(j * WAVE) + lin));
                    if constexpr (KV) v[j] = vin[sb + ((uint32_t)(j * WAVE) + lin)];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t x = k[j] ^ flip;  // padding: all ones
            a &= x;
            o |= ((uint32_t)j < nf || ((uint32_t)j == nf && tail_ok)) ? x : 0u;
        }
        const uint32_t diff = __builtin_amdgcn_readfirstlane(block_diff_bits<W>(a, o, sm.red_and, sm.red_or, lane, wid));
        lds_sort_passes(sm, k, v, diff, flip, ws0, atomic_rank, LeadingGroups{ng}, lane, wid);
        uint32_t nfs = nf, lout = lane;
        asm volatile("" : "+s"(nfs), "+v"(lout));
        if (nfs == (uint32_t)KPT) {
#pragma unroll
            for (int j = 0; j < KPT; ++j) out[sb + ((uint32_t)(j * WAVE) + lout)] = k[j];
            if constexpr (KV) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) vout[sb + ((uint32_t)(j * WAVE) + lout)] = v[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                if ((uint32_t)j < nfs || ((uint32_t)j == nfs && tail_ok)) {
                    out[sb + ((uint32_t)(j * WAVE) + lout)] = k[j];
                    if constexpr (KV) vout[sb + ((uint32_t)(j * WAVE) + lout)] = v[j];
                }
            }
        }
        __syncthreads();  // the next segment reuses red_and / red_or and the key slots
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

int cu_count() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
    }
    return cus;
}

unsigned stream_blocks(size_t n) {
    size_t b = (n + 256 * 8 - 1) / (256 * 8);
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

// The sort kernel of class c (0-2 wave, 3 block, 4 tile) over its list; vin/vout nullptr: keys only.
hipError_t launch_seg_sort(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                           const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                           hipStream_t s, const HySel &hy = HySel{}) {
    const bool kv = vin != nullptr;
    const unsigned cus = (unsigned)cu_count();
    // fixed grids, multiples of the CU count: what stays resident per CU by LDS
    if (c == 0) {
        if (kv) k_seg_wave<SEG_WAVE_KPT, true><<<cus * 8u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 0, flip, hy);
        else k_seg_wave<SEG_WAVE_KPT, false><<<cus * 8u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 0, flip, hy);
    } else if (c == 1) {
        if (kv) k_seg_wave<SEG_WAVE2_KPT, true><<<cus * 6u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 1, flip, hy);
        else k_seg_wave<SEG_WAVE2_KPT, false><<<cus * 8u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 1, flip, hy);
    } else if (c == 2) {  // 110-127 VGPRs: four waves per SIMD
        if (kv) k_seg_wave<SEG_WAVE3_KPT, true><<<cus * 4u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 2, flip, hy);
        else k_seg_wave<SEG_WAVE3_KPT, false><<<cus * 4u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 2, flip, hy);
    } else if (c == 3) {
        if (kv) k_seg_block<SEG_BLOCK, SEG_BLOCK_KPT, true, SEG_BLOCK_WPE><<<cus * 4u, SEG_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 3, flip, hy);
        else k_seg_block<SEG_BLOCK, SEG_BLOCK_KPT, false, SEG_BLOCK_WPE><<<cus * (unsigned)SEG_BLOCK_WGS, SEG_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 3, flip, hy);
    } else if (c == 4) {
        if (kv) k_seg_block<TS_BLOCK, TS_KPT_KV, true><<<cus, TS_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 4, flip, hy);
        else k_seg_block<TS_BLOCK, TS_KPT, false><<<cus, TS_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 4, flip, hy);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
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
                                  size_t stride, uint32_t flip, hipStream_t s) {
    size_t edges[SEG_CLASSES];
    labsort_segment_class_edges(pairs ? 1 : 0, edges, SEG_CLASSES);
    int ncls = 1;
    while (ncls < SEG_CLASSES && max_len > edges[ncls - 1]) ++ncls;
    for (int c = 0; c < ncls; ++c) {
        const hipError_t e = launch_seg_sort(c, in, out, vin, vout, off, hdr, lists + (size_t)c * stride, flip, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------------
// the hybrid radix sort's finish
// ---------------------------------------------------------------------------------
namespace {
constexpr int FB_BLOCK = 1024;  // buckets per workgroup of k_fin_bounds

// off[q] = first position whose key's top 16 bits are >= q, for the HY_BUCKETS buckets q, and
// off[HY_BUCKETS] = n.  The keys are ordered by their top 16 bits.  Bucket q lies in the range of
// its top-14-bit group q >> 2, which the exclusive scan of top14 gives: at most HY_MAX_BUCKET
// keys when the plan chose the hybrid path, so the search takes 15 steps, not 28.
__global__ __launch_bounds__(FB_BLOCK) void k_fin_bounds(const Plan *__restrict__ plan, Bufs bufs, uint32_t n, uint32_t flip,
                                                         const uint32_t *__restrict__ top14, uint32_t *__restrict__ off) {
    constexpr uint32_t GPB = FB_BLOCK / 4;  // top-14-bit groups per workgroup
    __shared__ uint32_t wsum[FB_BLOCK / WAVE];
    __shared__ uint32_t gstart[GPB + 1];
    if (plan->hybrid == 0u) return;
    const uint32_t *__restrict__ keys = bufs.p[plan->fin_src];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t g0 = blockIdx.x * GPB;  // this workgroup's first group
    // keys in the groups before g0, then the exclusive scan of this workgroup's groups
    uint32_t before = 0u;
    for (uint32_t i = tid; i < g0; i += FB_BLOCK) before += top14[i];
    const uint32_t mine = tid < GPB ? top14[g0 + tid] : 0u;
    uint32_t x = mine, tot = before;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(x, o);
        if (lane >= (uint32_t)o) x += t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (lane == 63u) wsum[wid] = x;
    __syncthreads();
    uint32_t pre = 0u;  // counts of the waves before this one (the groups sit in waves 0-3)
    for (uint32_t w = 0; w < wid && w < GPB / WAVE; ++w) pre += wsum[w];
    __syncthreads();
    if (lane == 0u) wsum[wid] = tot;
    __syncthreads();
    uint32_t base = 0u;
    for (uint32_t w = 0; w < (uint32_t)(FB_BLOCK / WAVE); ++w) base += wsum[w];
    if (tid < GPB) {
        gstart[tid] = base + pre + x - mine;
        if (tid == GPB - 1u) gstart[GPB] = base + pre + x;
    }
    __syncthreads();
    const uint32_t q = blockIdx.x * FB_BLOCK + tid;  // bucket
    uint32_t lo = min(gstart[tid >> 2], n), hi = min(gstart[(tid >> 2) + 1u], n);
    // (seven probes per round instead of one, 4 + 3 dependent rounds instead of 15, measured slower:
    // 78 us against 45 at 2^28 -- the probes are scattered single-word loads over 1 GiB, and their
    // number, not the length of the chain, is what costs)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (((keys[mid] ^ flip) >> 16) >= q) hi = mid;
        else lo = mid + 1u;
    }
    off[q] = lo;
    if (q == HY_BUCKETS - 1u) off[HY_BUCKETS] = n;
}
}  // namespace

hipError_t launch_hybrid_finish(const Plan *plan, Bufs b, size_t n, uint32_t flip, const uint32_t *top14, uint32_t *hdr,
                                uint32_t *off, uint32_t *lists, hipStream_t s) {
    static_assert(HY_BUCKETS % FB_BLOCK == 0 && HY_TOP * 4 == (int)HY_BUCKETS, "four buckets per top-14-bit group");
    const size_t stride = HY_BUCKETS;
    k_fin_bounds<<<HY_BUCKETS / FB_BLOCK, FB_BLOCK, 0, s>>>(plan, b, (uint32_t)n, flip, top14, off);
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
        if (c == 3) {  // the finish's own block class
            k_seg_block<HY_BLOCK, HY_BLOCK_KPT, false, HY_BLOCK_WPE><<<cus * (unsigned)HY_BLOCK_WPE, HY_BLOCK, 0, s>>>(
                out, out, nullptr, nullptr, off, hdr, list, 3, flip, hy);
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
    if (!key_type_ok(key_type)) return LABSORT_ERR_ARG;
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
        HIP_TRY(launch_seg_lds_classes(max_len, pairs, ki, ko, vi, vo, off, hdr, lists, L.list_stride, flip, s));
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
