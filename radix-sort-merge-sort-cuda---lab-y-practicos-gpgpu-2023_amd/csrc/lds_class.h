// lds_class.h -- what the LDS class kernels of the segmented sort (seg_kernels.h: k_seg_wave,
// k_seg_block) and of the dense row sort (rowsort.hip: k_rs_wave, k_rs_block) share.  DESIGN.md §3.13.
//
// A unit is what one wave (wave classes) or one workgroup (block and tile classes) sorts: a
// segment or a row, elements [b, b + len) of the caller's buffers.  The kernels keep what finds
// the unit (class lists and offsets, or row * cols); the block unit is written over a key policy:
//   uint32_t load(size_t i, uint32_t pos)      the sorted word of element i, position pos in its unit
//   uint32_t payload(size_t i, uint32_t pos)   the payload that follows it (key/value shapes)
//   void store_key(size_t i, uint32_t k), store_payload<KV>(size_t i, uint32_t k, uint32_t v)   element i of the outputs
//   static uint32_t diff(uint32_t d)           of the bits the words differ in, those that need a pass
// Words are ordered by (word ^ flip); padding is ~flip and sorts behind every key.
#pragma once
#include "devutil.h"
#include "lds_pass.h"

namespace labsort {

// ---- wave classes: one wave64 per unit, wave-private LDS, no workgroup barrier ----
template <int KPT, bool KV>
struct WaveSmem {
    uint32_t keys[WAVE * KPT];
    uint32_t vals[KV ? WAVE * KPT : 1];
    uint32_t hist[256];
    uint32_t probe[WAVE];
};

// One word per lane, len <= 64 of them: this lane's stable rank, the count of words before it
// in (word, lane) order.  Below len in lanes 0 .. len - 1.
__device__ __forceinline__ uint32_t wave_rank64(uint32_t x, uint32_t len, uint32_t lane) {
    uint32_t r = 0u;
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t xi = __builtin_amdgcn_readlane(x, (int)i);
        r += (xi < x || (xi == x && i < lane)) ? 1u : 0u;
    }
    return r;
}

// ---- block and tile classes: one workgroup per unit, the passes k_tile_sort runs (lds_sort_passes,
// lds_pass.h).  The unit is striped over the W waves in runs of S = 64 ceil(len / (64 W)) slots, so a short unit
// costs every wave the same few 64-key groups; groups past the end are neither ranked nor read back. ----
// A wave's stripe: nf whole 64-key groups and a last group of 1-63 keys or none, so whole groups
// load and store under scalar branches and one lane mask serves the last.  Wave-uniform but tail_ok.
struct Stripe {
    uint32_t ws0;  // the stripe's first slot in the unit and in LDS
    uint32_t nf;   // whole groups
    uint32_t ng;   // groups that hold keys: nf, or nf + 1 with the last group
    bool tail_ok;  // this lane holds a key of that last group
};
template <int W>
__device__ __forceinline__ Stripe block_stripe(uint32_t len, uint32_t lane, uint32_t wid) {
    const uint32_t jn = (len + (uint32_t)(W * WAVE) - 1u) / (uint32_t)(W * WAVE);  // groups per wave
    const uint32_t ws0 = wid * jn * WAVE;
    const uint32_t rem = ws0 < len ? len - ws0 : 0u;
    const uint32_t nf = min(jn, rem / WAVE);
    const uint32_t tail = nf < jn ? rem - nf * WAVE : 0u;  // < 64
    return {ws0, nf, nf + (tail ? 1u : 0u), lane < tail};
}

// One unit of the block or tile class, 1 <= len <= BLOCK * KPT, striped as `st`: loads, the bits
// the keys differ in, the passes, stores, and the barrier after which sm serves the next unit.
template <int BLOCK, int KPT, bool KV, class Keys>
__device__ __forceinline__ void block_sort_unit(TsSmem<BLOCK, KPT, KV> &sm, Keys io, size_t b, Stripe st,
                                                uint32_t flip, bool atomic_rank, uint32_t lane, uint32_t wid) {
    constexpr int W = TsSmem<BLOCK, KPT, KV>::W;
    const uint32_t ws0 = st.ws0, nf = st.nf;
    const bool tail_ok = st.tail_ok;
    // scalar base + 32-bit lane offset per access: the lane offsets pass through empty asms so no
    // 64-bit per-lane address is formed outside the caller's unit loop and held across it
    const size_t sb = b + ws0;
    uint32_t lin = lane;
    asm volatile("" : "+v"(lin));
    uint32_t k[KPT];
    uint32_t v[KV ? KPT : 1];
    uint32_t a = ~0u, o = 0u;
    // every load first, so all of them are in flight together (a use inside the scalar
    // branches would wait for each load in turn), then the bits the keys differ in
    if (nf == (uint32_t)KPT) {  // a whole tile: straight-line loads, as k_tile_sort
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t sl = (uint32_t)(j * WAVE) + lin;
            k[j] = io.load(sb + sl, ws0 + sl);
        }
        if constexpr (KV) {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint32_t sl = (uint32_t)(j * WAVE) + lin;
                v[j] = io.payload(sb + sl, ws0 + sl);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            uint32_t vj = 0u;
            k[j] = ~flip;
            if ((uint32_t)j < nf || ((uint32_t)j == nf && tail_ok)) {
                const uint32_t sl = (uint32_t)(j * WAVE) + lin;
                k[j] = io.load(sb + sl, ws0 + sl);
                if constexpr (KV) vj = io.payload(sb + sl, ws0 + sl);
            }
            if constexpr (KV) v[j] = vj;
        }
    }
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const uint32_t x = k[j] ^ flip;  // padding: all ones
        a &= x;
        o |= ((uint32_t)j < nf || ((uint32_t)j == nf && tail_ok)) ? x : 0u;
    }
    const uint32_t diff =
        Keys::diff(__builtin_amdgcn_readfirstlane(block_diff_bits<W>(a, o, sm.red_and, sm.red_or, lane, wid)));
    lds_sort_passes(sm, k, v, diff, flip, ws0, atomic_rank, LeadingGroups{st.ng}, lane, wid);
    uint32_t nfs = nf, lout = lane;
    asm volatile("" : "+s"(nfs), "+v"(lout));
    if (nfs == (uint32_t)KPT) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) io.store_key(sb + ((uint32_t)(j * WAVE) + lout), k[j]);
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            uint32_t vj = 0u;
            if constexpr (KV) vj = v[j];
            io.template store_payload<KV>(sb + ((uint32_t)(j * WAVE) + lout), k[j], vj);
        }
    } else {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            uint32_t vj = 0u;
            if constexpr (KV) vj = v[j];
            if ((uint32_t)j < nfs || ((uint32_t)j == nfs && tail_ok)) {
                io.store_key(sb + ((uint32_t)(j * WAVE) + lout), k[j]);
                io.template store_payload<KV>(sb + ((uint32_t)(j * WAVE) + lout), k[j], vj);
            }
        }
    }
    __syncthreads();  // the next unit reuses red_and / red_or and the key slots
}

}  // namespace labsort
