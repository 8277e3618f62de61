// seg_kernels.h -- the segmented sort's LDS class kernels and their launch, included by segsort.hip
// (integer keys, the hybrid radix finish) and segsort_f32.hip (float32 keys).  They keep what finds
// a segment; the block body, WaveSmem and the 64-key rank are lds_class.h's.  The wave classes' pass
// loop stands here and in rowsort.hip, word for word (why: DESIGN.md §3.13).  The float32
// instantiations have a translation unit of their own: with both sets in one device module the
// integer pair kernels of the block and tile classes came out with other register counts (88 -> 86
// and 101 -> 114 VGPRs) although their source is the same, and the integer paths are to compile to
// what they were (profiles/f32_keys.txt).
#pragma once
#include "segsort.h"

#include "devutil.h"
#include "host.h"
#include "lds_class.h"

namespace labsort {

namespace {

// F32 (float32 keys): a key becomes its order image right after its load and the word again
// right before its store; everything between orders uint32 words as it does for integer keys.
// The hybrid radix finish and the integer key types run the F32 = false instantiations.
template <bool F32>
__device__ __forceinline__ uint32_t seg_key_in(uint32_t w) {
    if constexpr (F32) return f32_ord(w);
    else return w;
}
template <bool F32>
__device__ __forceinline__ uint32_t seg_key_out(uint32_t k) {
    if constexpr (F32) return f32_unord(k);
    else return k;
}

// The key policy of lds_class.h: keys and payloads are 32-bit words of in / vin, every digit counts.
// NT: the streamed-load bit of the class (0: plain loads).
template <bool F32, int NT>
struct SegKeys {
    const uint32_t *in;
    uint32_t *out;
    const uint32_t *vin;
    uint32_t *vout;
    __device__ __forceinline__ uint32_t load(size_t i, uint32_t) const { return seg_key_in<F32>(ld_stream<NT>(in + i)); }
    __device__ __forceinline__ uint32_t payload(size_t i, uint32_t) const { return vin[i]; }
    __device__ __forceinline__ void store_key(size_t i, uint32_t k) const { out[i] = seg_key_out<F32>(k); }
    template <bool KV>
    __device__ __forceinline__ void store_payload(size_t i, uint32_t, uint32_t v) const {
        if constexpr (KV) vout[i] = v;
    }
    static __device__ __forceinline__ uint32_t diff(uint32_t d) { return d; }
};

// wave classes: one wave64 per segment, wave-private LDS, no workgroup barrier
template <int KPT, bool KV, bool F32 = false>
__global__ __launch_bounds__(SEG_WAVE_WPB * WAVE) void k_seg_wave(const uint32_t *in, uint32_t *out, const uint32_t *vin,
                                                                  uint32_t *vout, const uint32_t *__restrict__ off,
                                                                  const uint32_t *__restrict__ hdr,
                                                                  const uint32_t *__restrict__ list, int cls,
                                                                  uint32_t flip, HySel hy) {
    constexpr uint32_t CAP = WAVE * KPT;
    __shared__ WaveSmem<KPT, KV> sm_all[SEG_WAVE_WPB];
    if (hy.plan) {  // the radix sort's finish: the plan's choice first, and the buffer it names
        if (hy.plan->hybrid == 0u) return;
        in = hy.buf[hy.plan->fin_src];
    }
    if (ld_agent(hdr) != 0u) return;  // rejected offsets: touch nothing
    const uint32_t cnt = hdr[SEG_HDR_CNT + cls];
    const uint32_t lane = threadIdx.x & 63u, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (blockIdx.x * SEG_WAVE_WPB + wid >= cnt) return;  // (an empty class costs its launch only)
    WaveSmem<KPT, KV> &sm = sm_all[wid];
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
            const uint32_t x = ok ? (seg_key_in<F32>(in[b + lane]) ^ flip) : 0xFFFFFFFFu;
            uint32_t v = 0u;
            if constexpr (KV) v = ok ? vin[b + lane] : 0u;
            const uint32_t r = wave_rank64(x, len, lane);
            if (ok) {  // r < len: fewer than len keys come before one of them
                out[b + r] = seg_key_out<F32>(x ^ flip);
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
            k[j] = ok ? seg_key_in<F32>(in[b + idx]) : sentinel;
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
            if (idx < len) {
                out[b + idx] = seg_key_out<F32>(k[j]);
                if constexpr (KV) vout[b + idx] = v[j];
            }
        }
    }
}

// block and tile classes: block_sort_unit (lds_class.h) on each segment of the class list
template <int BLOCK, int KPT, bool KV, int WPE = 4, bool F32 = false>
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
    if (blockIdx.x >= cnt) return;  // (an empty class costs its launch only; uniform over the workgroup)
    probe_lane_order(sm.probe, &sm.ordered, lane, wid);
    __syncthreads();
    const bool atomic_rank = lane_order_probed(&sm.ordered);
    const SegKeys<F32, NT_TILE> io{in, out, vin, vout};
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
        block_sort_unit(sm, io, (size_t)b, block_stripe<W>(len, lane, wid), flip, atomic_rank, lane, wid);
    }
}

// The sort kernel of class c (0-2 wave, 3 block, 4 tile) over its list, in the shape and on the
// fixed grid that SEG_CLASS (segsort.h) gives; vin/vout nullptr: keys only.
template <bool F32>
hipError_t launch_seg_sort_t(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                             const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                             hipStream_t s, const HySel &hy) {
    const unsigned cus = (unsigned)cu_count();
    return seg_class_dispatch(c, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        constexpr SegClass g = SEG_CLASS[C];
        auto launch = [&](auto kernel, int wgs) {
            kernel<<<cus * (unsigned)wgs, g.block, 0, s>>>(in, out, vin, vout, off, hdr, list, C, flip, hy);
            return hipGetLastError();
        };
        if constexpr (C < 3)
            return vin ? launch(k_seg_wave<g.kpt_kv, true, F32>, g.wgs_kv) : launch(k_seg_wave<g.kpt, false, F32>, g.wgs);
        else
            return vin ? launch(k_seg_block<g.block, g.kpt_kv, true, g.wpe, F32>, g.wgs_kv)
                       : launch(k_seg_block<g.block, g.kpt, false, g.wpe, F32>, g.wgs);
    });
}

}  // namespace

// launch_seg_sort_t<true> (segsort_f32.hip)
hipError_t launch_seg_sort_f32(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                               const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                               hipStream_t s, const HySel &hy);

}  // namespace labsort
