// seg_kernels.h -- the segmented sort's LDS class kernels and their launch, included by segsort.hip
// (integer keys, the hybrid radix finish) and segsort_f32.hip (float32 keys).  The float32
// instantiations have a translation unit of their own: with both sets in one device module the
// integer pair kernels of the block and tile classes came out with other register counts (88 -> 86
// and 101 -> 114 VGPRs) although their source is the same, and the integer paths are to compile to
// what they were (profiles/f32_keys.txt).
#pragma once
#include "segsort.h"

#include "devutil.h"
#include "lds_pass.h"

namespace labsort {

namespace {

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

template <int KPT, bool KV, bool F32 = false>
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
            const uint32_t x = ok ? (seg_key_in<F32>(in[b + lane]) ^ flip) : 0xFFFFFFFFu;
            uint32_t v = 0u;
            if constexpr (KV) v = ok ? vin[b + lane] : 0u;
            uint32_t r = 0u;
            for (uint32_t i = 0; i < len; ++i) {
                const uint32_t xi = __builtin_amdgcn_readlane(x, (int)i);
                r += (xi < x || (xi == x && i < lane)) ? 1u : 0u;
            }
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
                out[b + idx] = seg_key_out<F32>(k[j]);
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
            for (int j = 0; j < KPT; ++j) k[j] = seg_key_in<F32>(ld_stream<NT_TILE>(in + sb + ((uint32_t)(j * WAVE) + lin)));
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
                    k[j] = seg_key_in<F32>(ld_stream<NT_TILE>(in + sb + ((uint32_t)(j * WAVE) + lin)));
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
            for (int j = 0; j < KPT; ++j) out[sb + ((uint32_t)(j * WAVE) + lout)] = seg_key_out<F32>(k[j]);
            if constexpr (KV) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) vout[sb + ((uint32_t)(j * WAVE) + lout)] = v[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                if ((uint32_t)j < nfs || ((uint32_t)j == nfs && tail_ok)) {
                    out[sb + ((uint32_t)(j * WAVE) + lout)] = seg_key_out<F32>(k[j]);
                    if constexpr (KV) vout[sb + ((uint32_t)(j * WAVE) + lout)] = v[j];
                }
            }
        }
        __syncthreads();  // the next segment reuses red_and / red_or and the key slots
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

// The sort kernel of class c (0-2 wave, 3 block, 4 tile) over its list; vin/vout nullptr: keys only.
template <bool F32>
hipError_t launch_seg_sort_t(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                             const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                             hipStream_t s, const HySel &hy) {
    const bool kv = vin != nullptr;
    const unsigned cus = (unsigned)cu_count();
    // fixed grids, multiples of the CU count: what stays resident per CU by LDS
    if (c == 0) {
        if (kv) k_seg_wave<SEG_WAVE_KPT, true, F32><<<cus * 8u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 0, flip, hy);
        else k_seg_wave<SEG_WAVE_KPT, false, F32><<<cus * 8u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 0, flip, hy);
    } else if (c == 1) {
        if (kv) k_seg_wave<SEG_WAVE2_KPT, true, F32><<<cus * 6u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 1, flip, hy);
        else k_seg_wave<SEG_WAVE2_KPT, false, F32><<<cus * 8u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 1, flip, hy);
    } else if (c == 2) {  // 110-127 VGPRs: four waves per SIMD
        if (kv) k_seg_wave<SEG_WAVE3_KPT, true, F32><<<cus * 4u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 2, flip, hy);
        else k_seg_wave<SEG_WAVE3_KPT, false, F32><<<cus * 4u, SEG_WAVE_WPB * WAVE, 0, s>>>(in, out, vin, vout, off, hdr, list, 2, flip, hy);
    } else if (c == 3) {
        if (kv) k_seg_block<SEG_BLOCK, SEG_BLOCK_KPT, true, SEG_BLOCK_WPE, F32><<<cus * 4u, SEG_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 3, flip, hy);
        else k_seg_block<SEG_BLOCK, SEG_BLOCK_KPT, false, SEG_BLOCK_WPE, F32><<<cus * (unsigned)SEG_BLOCK_WGS, SEG_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 3, flip, hy);
    } else if (c == 4) {
        if (kv) k_seg_block<TS_BLOCK, TS_KPT_KV, true, 4, F32><<<cus, TS_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 4, flip, hy);
        else k_seg_block<TS_BLOCK, TS_KPT, false, 4, F32><<<cus, TS_BLOCK, 0, s>>>(in, out, vin, vout, off, hdr, list, 4, flip, hy);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

// launch_seg_sort_t<true> (segsort_f32.hip)
hipError_t launch_seg_sort_f32(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                               const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                               hipStream_t s, const HySel &hy);

}  // namespace labsort
