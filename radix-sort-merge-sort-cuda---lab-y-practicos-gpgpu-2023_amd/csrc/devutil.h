// devutil.h -- wave64 / LDS device helpers shared by the labsort kernels (gfx950).
#pragma once
#include "common.h"

namespace labsort {

// ---------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Streamed key loads (NT_LOADS, one bit per kernel family, NT_*): a pass reads
// each key once, so its loads are issued nontemporal and the L2 keeps its capacity for
// the lines being written.  For the onesweep scatter that matters: the partial 64-B
// granules two consecutive tiles write at a digit-run boundary meet in the L2 before
// write-back instead of reaching HBM as read-modify-writes.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <int BIT>
__device__ __forceinline__ uint32_t ld_stream(const uint32_t *p) {
    if constexpr ((NT_LOADS & BIT) != 0) return __builtin_nontemporal_load(p);
    else return *p;
}
template <int BIT>
__device__ __forceinline__ uint4 ld_stream4(const uint4 *p) {
    if constexpr ((NT_LOADS & BIT) != 0) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}

// Lanes whose digit equals mine (all 64 lanes active): BITS ballots.
template <int BITS>
__device__ __forceinline__ uint64_t match_digit(uint32_t d) {
    uint64_t m = ~0ull;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// Lanes whose 8-bit digit equals mine, XOR form (v_xor / v_or3 per ballot).
__device__ __forceinline__ uint64_t match8(uint32_t d) {
    uint32_t xlo = 0, xhi = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int32_t sgn = ((int32_t)(d << (31 - b))) >> 31;  // 0 or -1: bit b of d
        const uint64_t bal = __ballot(sgn != 0);
        xlo |= (uint32_t)bal ^ (uint32_t)sgn;
        xhi |= (uint32_t)(bal >> 32) ^ (uint32_t)sgn;
    }
    return ((uint64_t)~xhi << 32) | (uint64_t)~xlo;
}

// Lanes of this wave whose digit selects the same LDS slot as mine, by an atomic XOR
// of lane bits: the slot changes by exactly the peers' bits whatever it held, so it
// needs no clearing (a read before and after instead of an OR, a read and a 64-bit
// clearing store).  LDS operations of one wave complete in issue order.
__device__ __forceinline__ uint64_t lds_peers(uint64_t *slot, uint32_t lane) {
    const uint64_t before = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_fetch_xor(slot, 1ull << lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return before ^ __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// True (in every lane) if one returning LDS atomic add instruction services the lanes
// that hit one address in ascending lane order, on five sharing patterns (all lanes,
// contiguous groups, strided groups, two scrambled ones).  Call with the whole wave
// active; `scratch` = 64 words of LDS private to the wave.
// LABSORT_RANK_FALLBACK=1 (A/B and test builds): answer false, so every kernel ranks by
// rank8's ballot path, which lane-ordered hardware otherwise never runs.
#ifndef LABSORT_RANK_FALLBACK
#define LABSORT_RANK_FALLBACK 0
#endif
__device__ __forceinline__ bool lds_lane_ordered(uint32_t *scratch, uint32_t lane) {
    if constexpr (LABSORT_RANK_FALLBACK != 0) return false;
    bool ok = true;
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        const uint32_t a = p == 0 ? 0u
                         : p == 1 ? lane >> 3
                         : p == 2 ? lane & 7u
                         : p == 3 ? ((lane * 37u) ^ (lane >> 2)) & 15u
                                  : ((lane * 0x9E37u) >> 5) & 3u;
        __hip_atomic_store(scratch + lane, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        const uint32_t got = __hip_atomic_fetch_add(scratch + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        ok &= got == mbcnt64(match_digit<6>(a));
    }
    return __ballot(!ok) == 0ull;
}

// Stable rank of digit d among this wave's keys so far, by one returning LDS atomic
// add on the wave's counter wh[d] (lane-ordered: see lds_lane_ordered).  A digit the
// whole wave shares (sorted or nearly sorted input: the high digits of 64 consecutive
// keys) takes one add of 64 instead of 64 adds serialised on one address.  All 64
// lanes active.
__device__ __forceinline__ uint32_t wave_atomic_rank(uint32_t *wh, uint32_t d, uint32_t lane) {
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    if (__ballot(d != d0) == 0ull) {
        uint32_t b = 0;
        if (lane == 0) b = __hip_atomic_fetch_add(wh + d0, 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        return __builtin_amdgcn_readfirstlane(b) + lane;
    }
    return __hip_atomic_fetch_add(wh + d, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Stable rank of 8-bit digit d among this wave's keys so far, on the wave's counters wh:
// the returning atomic where lanes are ordered (atomic_rank, wave-uniform), else the
// lanes with my digit by 8 ballots and one add by the first of them.  All 64 lanes active.
__device__ __forceinline__ uint32_t rank8(uint32_t *wh, uint32_t d, uint32_t lane, bool atomic_rank) {
    if (atomic_rank) return wave_atomic_rank(wh, d, lane);
    const uint64_t m = match8(d);
    const uint32_t pre = mbcnt64(m);
    const uint32_t old = wh[d];
    if (pre == 0) wh[d] = old + (uint32_t)__popcll(m);
    return old + pre;
}

// lds_lane_ordered once per workgroup: wave 0 probes (`scratch`: 64 LDS words) and
// publishes the answer in *flag; after the next barrier lane_order_probed reads it
// wave-uniformly.
__device__ __forceinline__ void probe_lane_order(uint32_t *scratch, uint32_t *flag, uint32_t lane, uint32_t wid) {
    if (wid == 0) {
        const bool ord = lds_lane_ordered(scratch, lane);
        if (lane == 0) *flag = ord ? 1u : 0u;
    }
}
__device__ __forceinline__ bool lane_order_probed(const uint32_t *flag) {
    return __builtin_amdgcn_readfirstlane(*flag) != 0u;
}

// Two 16-bit values (wave-local ranks, LDS slots) per register: value j of p.
template <int N>
__device__ __forceinline__ uint32_t get16(const uint32_t (&p)[N], int j) {
    return (p[j / 2] >> ((j & 1) * 16)) & 0xFFFFu;
}
template <int N>
__device__ __forceinline__ void set16(uint32_t (&p)[N], int j, uint32_t v) {
    __builtin_assume(v < 65536u);  // (spares the mask of a half that is filled first)
    p[j / 2] = (j & 1) ? (p[j / 2] & 0xFFFFu) | (v << 16) : (p[j / 2] & 0xFFFF0000u) | v;
}

// AND and OR of a value pair over the wave (all lanes get both); with a = o = key ^ flip
// over a set of keys, a ^ o is the bits the keys differ in.
__device__ __forceinline__ void wave_and_or(uint32_t &a, uint32_t &o) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a &= __shfl_xor(a, off);
        o |= __shfl_xor(o, off);
    }
}
// The bits the workgroup's keys differ in, from each lane's AND / OR: over the wave, then
// over the W waves through red_and / red_or (W words each).  Contains a barrier.
template <int W>
__device__ __forceinline__ uint32_t block_diff_bits(uint32_t a, uint32_t o, uint32_t *red_and, uint32_t *red_or,
                                                    uint32_t lane, uint32_t wid) {
    wave_and_or(a, o);
    if (lane == 0) {
        red_and[wid] = a;
        red_or[wid] = o;
    }
    __syncthreads();
    uint32_t aa = ~0u, oo = 0u;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        aa &= red_and[w];
        oo |= red_or[w];
    }
    return aa ^ oo;
}

// OR of a 64-bit pair over the wave (all lanes get both)
__device__ __forceinline__ void wave_or2(uint64_t &a, uint64_t &b) {
    uint32_t w[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] |= __shfl_xor(w[i], off);
    a = ((uint64_t)w[1] << 32) | w[0];
    b = ((uint64_t)w[3] << 32) | w[2];
}
// ... and over the workgroup's W waves, through red (2 * W words of 64 bits).  Contains a barrier.
template <int W>
__device__ __forceinline__ void block_or2(uint64_t &a, uint64_t &b, uint64_t *red, uint32_t lane, uint32_t wid) {
    wave_or2(a, b);
    if (lane == 0) {
        red[2 * wid] = a;
        red[2 * wid + 1] = b;
    }
    __syncthreads();
    a = 0ull;
    b = 0ull;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        a |= red[2 * w];
        b |= red[2 * w + 1];
    }
}

// Inclusive prefix sum of x over the wave's lanes (all 64 active).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(x, off);
        if (lane >= (uint32_t)off) x += t;
    }
    return x;
}

// Exclusive scan over the first R threads of the block (value v in thread tid < R,
// others pass 0).  Must be called by every thread (contains a barrier when R > 64).
template <int BLOCK, int R>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wsum) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t x = v;  // (wave_incl_scan, written out: through the helper k_onesweep's instruction text moves)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(x, off);
        if (lane >= (uint32_t)off) x += t;
    }
    if constexpr (R > 64) {
        constexpr int NW = R / 64;
        if (lane == 63 && wid < (uint32_t)NW) wsum[wid] = x;
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if ((uint32_t)w < wid) add += wsum[w];
        x += add;
    }
    return x - v;
}

// Digit d = tid < 256 of a tile ranked by W waves: its count over the waves and its first
// slot in the digit-ordered tile (meaningless in threads 256 and up).
struct DigitSpan {
    uint32_t tot, start;
};
// whist[w * 256 + d] = wave w's count of digit d on entry (complete: after a barrier),
// the first slot of wave w's keys of digit d on return (visible after the next barrier):
// with the tile-wide offsets folded in, the reorder reads one LDS word per key (r17).
// Must be called by every thread.
template <int BLOCK, int W>
__device__ __forceinline__ DigitSpan fold_digit_offsets(uint32_t *whist, uint32_t *wsum) {
    const uint32_t tid = threadIdx.x;
    uint32_t tot = 0;
    if (tid < 256u) {
#pragma unroll
        for (int w = 0; w < W; ++w) tot += whist[w * 256 + tid];
    }
    const uint32_t ds = block_excl_scan<BLOCK, 256>(tot, wsum);
    if (tid < 256u) {
        uint32_t run = ds;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t c = whist[w * 256 + tid];
            whist[w * 256 + tid] = run;
            run += c;
        }
    }
    return {tot, ds};
}

// Stable rank of KPT digits per lane inside one wave (slot-major order: slot j of
// lane l is element j*64+l of the wave's stripe).  `wh` = this wave's R counters
// (zeroed); on return wh[d] = count of digit d in the wave.
template <int BITS, int KPT>
__device__ __forceinline__ void wave_rank(const uint32_t (&dig)[KPT], uint32_t (&rank)[KPT], uint32_t *wh) {
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const uint32_t d = dig[j];
        const uint64_t m = match_digit<BITS>(d);
        const uint32_t pre = mbcnt64(m);
        const uint32_t old = wh[d];  // peers read the same word (broadcast)
        if (pre == 0) wh[d] = old + (uint32_t)__popcll(m);  // one leader per digit
        rank[j] = old + pre;
    }
}

// ---------------------------------------------------------------------------------
// aligned-group loads (the top-k select's and sort16's reads of a chunk of a row)
// ---------------------------------------------------------------------------------
// Elements [beg, end) of an array of 4- or 2-byte elements T are read in groups of
// E = 16 / sizeof(T) (quads, octs) that start 16-byte aligned: group q holds the elements
// i0 .. i0 + E - 1, i0 = beg - mis + E q, where mis = 0 .. E - 1 is how far element beg lies
// into its 16 bytes (base is aligned to T only; a row of odd length starts anywhere).
// group_mis: mis.  group_count: the groups that hold an element of the range.
template <typename T>
__device__ __forceinline__ uint32_t group_mis(const T *base, uint32_t beg) {
    return (uint32_t)(((uintptr_t)(base + beg) / sizeof(T)) & (16u / sizeof(T) - 1u));
}
template <int E>
__device__ __forceinline__ uint32_t group_count(uint32_t beg, uint32_t end, uint32_t mis) {
    return (end - beg + mis + (uint32_t)E - 1u) / (uint32_t)E;
}
// Group q < group_count: a group inside the range is one 16-byte load, the head and the tail
// are read element by element.  u[j] = map(element i0 + j) where it exists (0 elsewhere);
// returns the mask of those j.  map takes a uint32_t and, for 2-byte elements, must read its
// low half only (the high half holds the neighbour).
template <typename T, typename MAP>
__device__ __forceinline__ uint32_t load_group(const T *base, uint32_t beg, uint32_t end, uint32_t mis, uint32_t q,
                                               uint32_t (&u)[16 / sizeof(T)], int64_t &i0, MAP map) {
    constexpr int E = 16 / sizeof(T);
    static_assert(E == 4 || E == 8, "4- or 2-byte elements");
    i0 = (int64_t)beg - (int64_t)mis + E * (int64_t)q;
    if (i0 >= (int64_t)beg && i0 + E <= (int64_t)end) {
        const uint4 v = *reinterpret_cast<const uint4 *>(base + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (E == 4) {
                u[j] = map(w[j]);
            } else {
                u[2 * j] = map(w[j]);
                u[2 * j + 1] = map(w[j] >> 16);
            }
        }
        return (1u << E) - 1u;
    }
    uint32_t vm = 0u;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int64_t i = i0 + j;
        u[j] = 0u;
        if (i >= (int64_t)beg && i < (int64_t)end) {
            u[j] = map((uint32_t)base[i]);
            vm |= 1u << j;
        }
    }
    return vm;
}

// ---------------------------------------------------------------------------------
// slotted LDS digit histogram: h[digit * SLOTS + slot], 256 digits, slot = tid & (SLOTS - 1),
// so that the lanes of a wave that meet on one digit spread over SLOTS words
// ---------------------------------------------------------------------------------
// Clears h; the caller's barrier follows.
template <int SLOTS, int BLOCK>
__device__ __forceinline__ void slot_hist_clear(uint32_t *h, uint32_t tid) {
    for (uint32_t i = tid; i < 256u * SLOTS; i += BLOCK) h[i] = 0u;
}
// One key of thread tid.
template <int SLOTS>
__device__ __forceinline__ void slot_hist_add(uint32_t *h, uint32_t digit, uint32_t tid) {
    atomicAdd(&h[digit * SLOTS + (tid & (SLOTS - 1u))], 1u);
}
// Digit d's count (after a barrier): its slots, read from a start rotated by d so that
// neighbouring threads read different banks.
template <int SLOTS>
__device__ __forceinline__ uint32_t slot_hist_fold(const uint32_t *h, uint32_t d) {
    static_assert((SLOTS & (SLOTS - 1)) == 0, "a power of two");
    uint32_t sum = 0u;
#pragma unroll 8
    for (uint32_t q = 0; q < (uint32_t)SLOTS; ++q) sum += h[d * SLOTS + ((q + d) & (SLOTS - 1u))];
    return sum;
}

}  // namespace labsort
